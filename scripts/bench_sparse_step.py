#!/usr/bin/env python3
"""The shared-negative train step under optimizer_mode "dense" and "sparse" as the entity table grows: SharedNegatives(256) on ComplEx
k = 200 (multiclass_nll) and SharedDistanceNegatives(256) on RotatE k = 200 (self_adversarial), B = 10 000, G = M = 256, Adam,
N = 14 505 (the synthetic FB15k-237 sizes), 1 M and 4 M entities, R = 237.  Positives are uniform random triples over the N entities.

  dense  : amdkge_sample_shared -> the sampler's fwdbwd -> amdkge_opt_step over both tables (what StepLoop.step runs)
  sparse : amdkge_sample_shared -> the same fwdbwd -> amdkge_step_rows -> amdkge_opt_step_rows on the candidate rows + the row-wise
           sweep of the relation table (KgeEngine.opt_step_rows: what StepLoop.step runs with optimizer.sparse)

Method: HIP events around each step, `--warmup` untimed steps per configuration, then `--reps` timed steps, the two modes ALTERNATING
step by step on one engine; the median is reported with the minimum and the maximum.  The sparse step carries two more events, so the
two new calls are also reported alone: step_rows, and the sweep (entity rows + the relation table's 237 rows).  The sweep's bytes are
counted from the rows it moved, read once from the device in an untimed step: a candidate row without gradient costs one read of its
gradient row; a row with gradient is read in x, g and the two Adam slots and written in all four (its first gradient read hits HBM, the
second the cache): 8 streams of row_floats * 4 bytes.  bytes/s = those bytes over the sweep's median time.

usage: bench_sparse_step.py [--models ComplEx RotatE] [--N 14505 1000000 4000000] [--reps 20] [--warmup 3] [--out profiles/sparse_step.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {"ComplEx": ("multiclass_nll", False), "RotatE": ("self_adversarial", True)}   # model -> (loss, distance tiles)
LOSS_PARAMS = {"multiclass_nll": (0.0, 0.0), "self_adversarial": (3.0, 0.5)}             # (margin, alpha): the defaults of the loss classes
K_UNITS, B, M, R = 200, 10000, 256, 237


def stats(ms):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def run(models, Ns, reps, warmup):
    import torch

    from ampligraph_amd import _ffi
    from ampligraph_amd.engine import KgeEngine

    out = {"k": K_UNITS, "B": B, "M": M, "G": M, "R": R, "optimizer": "adam", "results": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for model in models:
        loss_name, distance = CONFIGS[model]
        loss = _ffi.Loss(_ffi.LOSSES[loss_name], 0, *LOSS_PARAMS[loss_name])
        for N in Ns:
            eng = KgeEngine(model, K_UNITS, N, R, max_rel_size=R)
            eng.ent.uniform_(-0.02, 0.02)       # (device-side fill: a host table of 4 M rows is 6.4 GB)
            eng.rel.uniform_(-0.1, 0.1)
            eng.prepare_training("adam")
            fwdbwd = eng.train_shared_dist_fwdbwd if distance else eng.train_shared_fwdbwd
            g = torch.Generator(device="cuda").manual_seed(N)
            nb = 8
            X = torch.stack([torch.randint(0, N, (nb * B,), device="cuda", generator=g), torch.randint(0, R, (nb * B,), device="cuda", generator=g),
                             torch.randint(0, N, (nb * B,), device="cuda", generator=g)], 1).int().contiguous()
            t = {"dense": [], "sparse": [], "step_rows": [], "sweep": []}
            counts = None
            for s in range(-warmup, reps):
                xb = X[(s % nb) * B:(s % nb + 1) * B]
                for mode in ("dense", "sparse"):
                    o = _ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, 2 * (s + warmup) + 1 + (mode == "sparse"))
                    ev[0].record()
                    ids, side = eng.sample_shared(xb, M, M, 0, s + warmup)
                    fwdbwd(xb, M, M, ids, side, loss)
                    if mode == "dense":
                        eng.opt_step(o)
                        ev[3].record()
                    else:
                        ev[1].record()
                        rows, n_rows = eng.step_rows(xb, ids)
                        ev[2].record()
                        if s == -1:   # (untimed) what the sweep is about to move
                            torch.cuda.synchronize()
                            n = int(n_rows.item())
                            counts = {"candidate_rows": n, "rows_with_gradient": int((eng.g_ent[rows[:n].long()] != 0).any(1).sum().item())}
                        eng.opt_step_rows(o, None, None, rows, n_rows, int(rows.numel()))
                        ev[3].record()
                    torch.cuda.synchronize()
                    if s >= 0:
                        t[mode].append(ev[0].elapsed_time(ev[3]))
                        if mode == "sparse":
                            t["step_rows"].append(ev[1].elapsed_time(ev[2]))
                            t["sweep"].append(ev[2].elapsed_time(ev[3]))
            assert not bool(eng.g_flat.any()), "the gradient tables are not zero after the last step"
            res = {"model": model, "loss": loss_name, "N": N, "row_floats": eng.Ks, "table_bytes": 4 * N * eng.Ks,
                   "dense": stats(t["dense"]), "sparse": stats(t["sparse"]), "step_rows": stats(t["step_rows"]), "sweep": stats(t["sweep"])}
            res.update(counts or {})
            if counts:
                moved = 4 * eng.Ks * (8 * counts["rows_with_gradient"] + (counts["candidate_rows"] - counts["rows_with_gradient"]))
                res["sweep"].update(bytes_moved=moved, bytes_per_s=moved / (res["sweep"]["ms"] * 1e-3))
            res["dense_over_sparse"] = res["dense"]["ms"] / res["sparse"]["ms"]
            out["results"].append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)
            del eng, X
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=list(CONFIGS), choices=list(CONFIGS))
    ap.add_argument("--N", type=int, nargs="+", default=[14505, 1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    if not torch.cuda.is_available():
        sys.exit("bench_sparse_step: needs a GPU (no CPU fallback)")
    out = run(a.models, a.N, a.reps, a.warmup)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

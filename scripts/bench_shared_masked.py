#!/usr/bin/env python3
"""The masked shared-negative step and the all-entities list at the C2 shape (synthetic FB15k-237 sizes: N = 14 505, R = 237, ComplEx
k = 200, B = 10 000, multiclass_nll), by the method of scripts/bench_shared_negatives.py: HIP events around each step, `--warmup`
untimed steps per configuration, then `--reps` timed steps; median with minimum and maximum.

Configurations (a step = the draw, the forward / backward and amdkge_opt_step):
  M1024_unmasked            sample_shared + train_shared_fwdbwd, G = M = 1 024          (runs on a build of the parent too)
  M1024_masked              the same ids through train_shared_masked_fwdbwd, ranges of the training set (GIVEN mode)
  all_unmasked_G{g}         the list 0 .. N - 1 for every group, only the sides drawn   (runs on a build of the parent too)
  all_masked_identity_G{g}  ... masked, AMDKGE_SHARED_LIST_IDENTITY
  all_masked_given_G{g}     ... masked, AMDKGE_SHARED_LIST_GIVEN on the same arange list
for g in --G (default 256 1024 4096).  The range arrays of all training rows are made once, outside the timed region, as
SharedNegatives.bind() makes them.  `--root DIR` imports the package from another tree (a build of the parent commit): the
configurations that need the masked entry points are then reported as skipped.

`--mrr` instead prints the filtered MRR of a short fit() on tests/planted.py's graph with {"shared": "all"} with and without
mask_known (same seeds, same epochs): the feature's purpose made visible, not a bar.

usage: bench_shared_masked.py [--root DIR] [--G 256 1024 4096] [--only NAME ...] [--reps 20] [--warmup 3] [--tag TEXT] [--out FILE]
       bench_shared_masked.py --mrr [--seeds 0 1 2] [--epochs 40] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL, K_UNITS, B, M_SAMPLED = "ComplEx", 200, 10000, 1024


def summary(ms):
    return {"ms_per_step": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def run(Gs, only, reps, warmup):
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.engine import KgeEngine

    d = make_synthetic_kg()
    N, R = d["n_ents"], d["n_rels"]
    eng = KgeEngine(MODEL, K_UNITS, N, R, max_rel_size=R)
    rng = np.random.default_rng(0)
    eng.set_tables(rng.uniform(-.02, .02, (N, eng.K)).astype(np.float32), rng.uniform(-.1, .1, (R, eng.K)).astype(np.float32))
    eng.prepare_training("adam")
    loss = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
    X = torch.as_tensor(d["train"]).cuda()
    nb = int(X.shape[0]) // B
    has_mask = hasattr(eng, "train_shared_masked_fwdbwd")
    sf = of = None
    if has_mask:
        index = FilterIndex([X], N, R, engine=eng)
        sf, of = index.device_filter(eng, X, "s"), index.device_filter(eng, X, "o")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    out = {"model": MODEL, "k": K_UNITS, "B": B, "N": N, "R": R, "loss": "multiclass_nll", "has_masked_entry_points": has_mask, "results": []}
    configs = [("M1024_unmasked", M_SAMPLED, M_SAMPLED, None), ("M1024_masked", M_SAMPLED, M_SAMPLED, "given")]
    for g in Gs:
        configs += [(f"all_unmasked_G{g}", N, g, None), (f"all_masked_identity_G{g}", N, g, "identity"), (f"all_masked_given_G{g}", N, g, "given")]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for name, M, G, mask in configs:
        if only and name not in only:
            continue
        if mask and not has_mask:
            out["results"].append({"name": name, "skipped": "this build has no masked entry points"})
            continue
        all_ids = None
        if M == N:
            all_ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(-(-B // min(G, B)), 1).contiguous()   # once, as bind() does
        ms = []
        stats.zero_()
        for s in range(-warmup, reps):
            r0 = (s % nb) * B
            xb = X[r0:r0 + B]
            o = _ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, s + warmup + 1)
            ev[0].record()
            if all_ids is None:
                ids, side = eng.sample_shared(xb, G, M, 0, s + warmup)
            else:
                ids, side = all_ids, eng.sample_shared(xb, G, 1, 0, s + warmup)[1]
            if mask:
                cut = lambda f: (f[0][r0:r0 + B], f[1][r0:r0 + B], f[2])   # noqa: E731
                eng.train_shared_masked_fwdbwd(xb, G, M, ids, side, loss, s_filter=cut(sf), o_filter=cut(of), identity=mask == "identity", stats=stats)
            else:
                eng.train_shared_fwdbwd(xb, G, M, ids, side, loss)
            eng.opt_step(o)
            ev[1].record()
            torch.cuda.synchronize()
            if s >= 0:
                ms.append(ev[0].elapsed_time(ev[1]))
        res = dict(summary(ms), name=name, M=M, G=G, mask=mask)
        if mask:
            mk, un = stats.tolist()
            res.update(masked_per_step=mk / (reps + warmup), unmaskable_per_step=un / (reps + warmup))
        out["results"].append(res)
        print(json.dumps(res), flush=True)
    return out


def run_mrr(seeds, epochs):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from planted import planted_kg

    from ampligraph_amd.evaluation.metrics import mrr_score
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    out = {"graph": "tests/planted.py planted_kg('ComplEx')", "model": "ComplEx", "k": 16, "loss": "multiclass_nll", "lr": 2e-2, "batch_size": 1024, "epochs": epochs, "results": []}
    for seed in seeds:
        d = planted_kg("ComplEx", seed=seed)
        train, test = d["train"].astype(str), d["test"].astype(str)
        row = {"seed": seed}
        for name, neg in (("unmasked", {"shared": "all"}), ("masked", {"shared": "all", "mask_known": True})):
            m = ScoringBasedEmbeddingModel(eta=5, k=16, scoring_type="ComplEx", seed=seed)
            m.compile(optimizer=optimizers.get("adam", {"learning_rate": 2e-2}), loss="multiclass_nll", negatives=neg)
            h = m.fit(train, batch_size=1024, epochs=epochs, verbose=False)
            ranks = m.evaluate(test, use_filter={"train": train, "test": test}, corrupt_side="s,o", verbose=False)
            row[name] = {"filtered_mrr": float(mrr_score(ranks)), "last_loss": float(h.history["loss"][-1])}
            if hasattr(m, "negative_sampling_stats_"):
                row[name]["stats"] = m.negative_sampling_stats_
        out["results"].append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT, help="the tree the package is imported from (default: this one)")
    ap.add_argument("--G", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--only", nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default=None, help="free text kept in the output (which build this is)")
    ap.add_argument("--mrr", action="store_true")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if not torch.cuda.is_available():
        sys.exit("bench_shared_masked: needs a GPU (no CPU fallback)")
    out = run_mrr(a.seeds, a.epochs) if a.mrr else run(a.G, a.only, a.reps, a.warmup)
    if a.tag:
        out["tag"] = a.tag
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The labelled (KvsAll) shared step at the C2 shape (synthetic FB15k-237 sizes: N = 14 505, R = 237, k = 200, B = 10 000, the
all-entities list in groups of G = 4 096), by the method of scripts/bench_shared_masked.py: HIP events around each step, `--warmup`
untimed steps per configuration, then `--reps` timed steps; median with minimum and maximum, one process.

Configurations, for ComplEx (matrix products) and TransE (distance tiles); a step = the side draw, the forward / backward and
amdkge_opt_step:
  {model}_labelled          train_shared_labels_fwdbwd / train_shared_dist_labels_fwdbwd: BCE, label_smoothing 0.1, IDENTITY list
  {model}_labelled_query    ... with the row weights of weight="query"
  {model}_masked_nll        the step it is the sibling of: the same list, mask_known + multiclass_nll (shared_mask_kernel, then
                            shared_loss_kernel)
and the kernels alone on one chunk's buffer [G, N] of ComplEx-sized scores, refilled before every repetition:
  kernel_label_loss         amdkge_shared_label_loss (labels + BCE, one pass): ms, and bytes/s against one read + one write of the buffer
  kernel_mask               amdkge_shared_mask_scores on the same buffer and ranges (the first of the pair it replaces)
shared_loss_kernel has no entry point of its own: the pair is compared through the two step configurations.

usage: bench_shared_labels.py [--G 4096] [--only NAME ...] [--reps 20] [--warmup 3] [--tag TEXT] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_UNITS, B = 200, 10000


def summary(ms):
    return {"ms_per_step": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed(fn, reps, warmup, before=None):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for s in range(-warmup, reps):
        if before is not None:
            before()
        ev[0].record()
        fn(s + warmup)
        ev[1].record()
        torch.cuda.synchronize()
        if s >= 0:
            ms.append(ev[0].elapsed_time(ev[1]))
    return ms


def run(G, only, reps, warmup):
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features.negatives import KvsAll

    d = make_synthetic_kg()
    N, R = d["n_ents"], d["n_rels"]
    X = torch.as_tensor(d["train"]).cuda()
    nb = int(X.shape[0]) // B
    out = {"k": K_UNITS, "B": B, "N": N, "R": R, "G": G, "label_smoothing": 0.1, "results": []}
    nll = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
    all_ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(-(-B // min(G, B)), 1).contiguous()   # once, as bind() does
    w_all = tuple(torch.as_tensor(w).cuda() for w in KvsAll.query_weights(d["train"]))
    sf = of = None
    for model in ("ComplEx", "TransE"):
        eng = KgeEngine(model, K_UNITS, N, R, max_rel_size=R)
        rng = np.random.default_rng(0)
        eng.set_tables(rng.uniform(-.02, .02, (N, eng.K)).astype(np.float32), rng.uniform(-.1, .1, (R, eng.K)).astype(np.float32))
        eng.prepare_training("adam")
        if sf is None:
            index = FilterIndex([X], N, R, engine=eng)
            sf, of = index.device_filter(eng, X, "s"), index.device_filter(eng, X, "o")
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
        dist = model == "TransE"
        labelled = eng.train_shared_dist_labels_fwdbwd if dist else eng.train_shared_labels_fwdbwd
        masked = eng.train_shared_dist_fwdbwd if dist else eng.train_shared_masked_fwdbwd

        def step(s, kind):
            r0 = (s % nb) * B
            xb = X[r0:r0 + B]
            cut = lambda f: (f[0][r0:r0 + B], f[1][r0:r0 + B], f[2])   # noqa: E731
            side = eng.sample_shared(xb, G, 1, 0, s)[1]
            if kind == "masked_nll":
                masked(xb, G, N, all_ids, side, nll, s_filter=cut(sf), o_filter=cut(of), identity=True, stats=stats)
            else:
                w = (w_all[0][r0:r0 + B], w_all[1][r0:r0 + B]) if kind == "labelled_query" else None
                labelled(xb, G, N, all_ids, side, cut(sf), cut(of), label_smoothing=0.1, reduction="sum", weights=w, identity=True, stats=stats)
            eng.opt_step(_ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, s + 1))

        for kind in ("labelled", "labelled_query", "masked_nll"):
            name = f"{model}_{kind}"
            if only and name not in only:
                continue
            stats.zero_()
            ms = timed(lambda s, kind=kind: step(s, kind), reps, warmup)
            a, b = stats.tolist()
            res = dict(summary(ms), name=name, model=model, M=N, G=G, stats_per_step=[a / (reps + warmup), b / (reps + warmup)])
            out["results"].append(res)
            print(json.dumps(res), flush=True)
        if model == "ComplEx":   # the kernels alone, on the first chunk's buffer: rows [0, G) of the first batch
            rows = min(G, B)
            S0 = (torch.randn(rows, N, device="cuda") * 2).contiguous()
            S = torch.empty_like(S0)
            xb = X[:B]
            side = eng.sample_shared(xb, G, 1, 0, 0)[1].clone()
            cut = lambda f: (f[0][:B], f[1][:B], f[2])   # noqa: E731
            acc = torch.zeros(1, dtype=torch.float64, device="cuda")
            kernels = (("kernel_label_loss", lambda s: eng.shared_label_loss(S, 0, G, None, side, cut(sf), cut(of), label_smoothing=0.1, reduction="sum",
                                                                             identity=True, loss_sum=acc, stats=stats)),
                       ("kernel_mask", lambda s: eng.shared_mask_scores(S, 0, G, None, side, cut(sf), cut(of), identity=True, stats=stats)))
            for name, fn in kernels:
                if only and name not in only:
                    continue
                ms = timed(fn, reps, warmup, before=lambda: S.copy_(S0))
                res = dict(summary(ms), name=name, rows=rows, M=N, buffer_bytes=4 * rows * N)
                if name == "kernel_label_loss":
                    res["read_plus_write_bytes_per_s"] = 2 * 4 * rows * N / (res["ms_per_step"] * 1e-3)
                out["results"].append(res)
                print(json.dumps(res), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=4096)
    ap.add_argument("--only", nargs="+", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default=None, help="free text kept in the output (which build this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        sys.exit("bench_shared_labels: needs a GPU (no CPU fallback)")
    out = run(a.G, a.only, a.reps, a.warmup)
    if a.tag:
        out["tag"] = a.tag
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The relation-prediction term (compile(relation_prediction=...): amdkge_train_relation_fwdbwd, multiclass_nll, known=True, weight
0.25) at the C2 shape (synthetic FB15k-237 sizes: N = 14 505, R = 237, k = 200, B = 10 000) for ComplEx, DistMult and HolE, by the method
of scripts/bench_batch_reg.py: HIP events around each step, `--warmup` untimed steps per configuration, then timed steps; median with
minimum and maximum.  A step = the draw (shared configurations), the forward / backward, the pair-range lookup and
amdkge_train_relation_fwdbwd where the configuration has the term, and amdkge_opt_step.

Every group holds one step WITHOUT the term -- the calls the parent commit makes, on device code the parent has
-- and the same step with it; the members of a group alternate in blocks of `--block` steps inside one process, so that what else
the machine does falls on all of them alike.

  shared_M256      sample_shared + train_shared_fwdbwd, G = M = 256, multiclass_nll            | + the term
  shared_all       the all-entities list, G = 4 096, masked (IDENTITY), multiclass_nll          | + the term
  per_corruption   trainer.StepLoop at eta = 20, self_adversarial (bench.py's C2 step):
                   the owner-computes step | the dense-gradient step (AMDKGE_TRAIN_PATH=atomic) | the dense-gradient step + the term
                   (the term takes the dense-gradient step: the owner-computes one never materialises an entity gradient)
  term_alone       amdkge_pair_filter_ranges + amdkge_train_relation_fwdbwd, nothing else

`--no-term` runs the members without the term only, and uses no entry point the parent commit lacks: with a library built from the
parent bound in place of this commit's, it times the parent's device code.

usage: bench_relation_objective.py [--model ComplEx ...] [--only GROUP ...] [--variant NAME] [--no-term] [--rounds 4] [--block 5] [--warmup 3]
                                   [--weight 0.25] [--out FILE]
       (--variant: run ONE member of each group without alternating -- for a profiler run)"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K_UNITS, B, ETA = 200, 10000, 20
GROUPS = ["shared_M256", "shared_all", "per_corruption", "term_alone"]


def summary(ms):
    return {"ms_per_step": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "steps": len(ms)}


def new_engine(model, N, R):
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(model, K_UNITS, N, R, max_rel_size=R)
    rng = np.random.default_rng(0)
    eng.set_tables(rng.uniform(-.02, .02, (N, eng.K)).astype(np.float32), rng.uniform(-.1, .1, (R, eng.K)).astype(np.float32))
    return eng


class Term:
    """what latent_features.relation_prediction.BoundRelationPrediction does per step, on an index over the whole training set"""

    def __init__(self, eng, X, N, R, weight):
        from ampligraph_amd import _ffi
        from ampligraph_amd.datasets.filters import PairFilterIndex

        self.eng, self.weight = eng, weight
        self.index = PairFilterIndex([X], N, R, engine=eng)
        self.loss = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
        self.stats = torch.zeros(2, dtype=torch.int64, device="cuda")

    def step(self, xb):
        self.eng.train_relation_fwdbwd(xb, self.loss, self.weight, flt=self.index.device_filter(self.eng, xb), stats=self.stats)


def shared_variants(model, d, X, which, weight, want_term):
    """-> {name: step(s)} for the shared group `which`; one engine serves both members"""
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex

    N, R = d["n_ents"], d["n_rels"]
    eng = new_engine(model, N, R)
    eng.prepare_training("adam")
    loss = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
    nb = int(X.shape[0]) // B
    term = Term(eng, X, N, R, weight) if want_term else None
    if which == "shared_all":
        G, M = 4096, N
        index = FilterIndex([X], N, R, engine=eng)
        sf, of = index.device_filter(eng, X, "s"), index.device_filter(eng, X, "o")
        all_ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(-(-B // G), 1).contiguous()
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    else:
        G = M = 256

    def step(s, with_term, main=True):
        r0 = (s % nb) * B
        xb = X[r0:r0 + B]
        o = _ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, s + 1)
        if not main:
            term.step(xb)
            return
        if which == "shared_all":
            side = eng.sample_shared(xb, G, 1, 0, s)[1]
            cut = lambda f: (f[0][r0:r0 + B], f[1][r0:r0 + B], f[2])   # noqa: E731
            eng.train_shared_masked_fwdbwd(xb, G, M, all_ids, side, loss, s_filter=cut(sf), o_filter=cut(of), identity=True, stats=stats)
        else:
            ids, side = eng.sample_shared(xb, G, M, 0, s)
            eng.train_shared_fwdbwd(xb, G, M, ids, side, loss)
        if with_term:
            term.step(xb)
        eng.opt_step(o)

    if which == "term_alone":
        return {"term": lambda s: step(s, True, main=False)}
    out = {"none": lambda s: step(s, False)}
    if want_term:
        out["term"] = lambda s: step(s, True)
    return out


def per_corruption_variants(model, d, X, weight, want_term):
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    N, R = d["n_ents"], d["n_rels"]
    nb = int(X.shape[0]) // B
    out = {}
    for name, with_term, path in (("owner_computes", False, ""), ("dense", False, "atomic"), ("dense_term", True, "")):
        if with_term and not want_term:
            continue
        os.environ["AMDKGE_TRAIN_PATH"] = path   # (read once, when the loop is made)
        eng = new_engine(model, N, R)
        loop = StepLoop(eng, ETA, loss_functions.get("self_adversarial"), optimizers.get("adam"), None, seed=0, dist=None)
        os.environ.pop("AMDKGE_TRAIN_PATH")
        assert loop.use_tiled == (path != "atomic")
        if with_term:
            loop.relation = Term(eng, X, N, R, weight)
        out[name] = (lambda s, loop=loop: loop.step(X[(s % nb) * B:(s % nb) * B + B], s))
    return out


def time_group(variants, rounds, block, warmup):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = {name: [] for name in variants}
    counters = {name: 0 for name in variants}

    def run(name, timed):
        s = counters[name]
        counters[name] += 1
        ev[0].record()
        variants[name](s)
        ev[1].record()
        torch.cuda.synchronize()
        if timed:
            ms[name].append(ev[0].elapsed_time(ev[1]))

    for name in variants:
        for _ in range(warmup):
            run(name, False)
    for _ in range(rounds):
        for name in variants:
            for _ in range(block):
                run(name, True)
    return {name: summary(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", nargs="+", default=["ComplEx", "DistMult", "HolE"], choices=["ComplEx", "DistMult", "HolE"])
    ap.add_argument("--only", nargs="+", default=None, choices=GROUPS)
    ap.add_argument("--variant", default=None)
    ap.add_argument("--no-term", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--weight", type=float, default=0.25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_relation_objective: needs a GPU (no CPU fallback)")
    from ampligraph_amd.datasets import make_synthetic_kg

    d = make_synthetic_kg()
    X = torch.as_tensor(d["train"]).cuda()
    want_term = not a.no_term and a.variant in (None, "term", "dense_term")
    out = {"k": K_UNITS, "B": B, "N": d["n_ents"], "R": d["n_rels"], "weight": a.weight, "rounds": a.rounds, "block": a.block, "models": {}}
    for model in a.model:
        res = out["models"][model] = {}
        for group in a.only or GROUPS:
            if group == "term_alone" and not want_term:
                continue
            variants = per_corruption_variants(model, d, X, a.weight, want_term) if group == "per_corruption" else shared_variants(model, d, X, group, a.weight, want_term)
            if a.variant:
                variants = {k: v for k, v in variants.items() if k == a.variant}
                if not variants:
                    continue
            res[group] = time_group(variants, a.rounds, a.block, a.warmup)
            print(json.dumps({model: {group: res[group]}}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

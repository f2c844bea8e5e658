#!/usr/bin/env python3
"""The batch regulariser (N3: BatchLPRegularizer(3, lambda), modulus norm on both tables) at the C2 shape (synthetic FB15k-237 sizes:
N = 14 505, R = 237, ComplEx k = 200, B = 10 000), by the method of scripts/bench_shared_negatives.py: HIP events around each step,
`--warmup` untimed steps per configuration, then timed steps; median with minimum and maximum.  A step = the draw (shared
configurations), the forward / backward, amdkge_batch_reg_fwdbwd where the configuration has the regulariser, and amdkge_opt_step.

Every group holds one step WITHOUT the regulariser -- the calls the parent commit makes, on device code the parent has (DESIGN.md
section 8) -- and the same step with it; the members of a group alternate in blocks of `--block` steps inside one process, so that
what else the machine does falls on all of them alike.

  shared_M256      sample_shared + train_shared_fwdbwd, G = M = 256, multiclass_nll            | + N3
  shared_all       the all-entities list, G = 4 096, masked (IDENTITY), multiclass_nll          | + N3
  per_corruption   trainer.StepLoop at eta = 20, self_adversarial (bench.py's C2 step):
                   the owner-computes step | the dense-gradient step (AMDKGE_TRAIN_PATH=atomic) | the dense-gradient step + N3
                   (a batch regulariser takes the dense-gradient step: the owner-computes one never materialises an entity gradient)

usage: bench_batch_reg.py [--only GROUP ...] [--variant NAME] [--rounds 4] [--block 5] [--warmup 3] [--lam 1e-3] [--out FILE]
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
MODEL, K_UNITS, B, ETA = "ComplEx", 200, 10000, 20


def summary(ms):
    return {"ms_per_step": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "steps": len(ms)}


def new_engine(N, R):
    from ampligraph_amd.engine import KgeEngine

    eng = KgeEngine(MODEL, K_UNITS, N, R, max_rel_size=R)
    rng = np.random.default_rng(0)
    eng.set_tables(rng.uniform(-.02, .02, (N, eng.K)).astype(np.float32), rng.uniform(-.1, .1, (R, eng.K)).astype(np.float32))
    return eng


def shared_variants(d, X, which, n3):
    """-> {name: step(s)} for the shared group `which`; one engine serves both members"""
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex

    N, R = d["n_ents"], d["n_rels"]
    eng = new_engine(N, R)
    eng.prepare_training("adam")
    loss = _ffi.Loss(_ffi.LOSSES["multiclass_nll"], 0, 0.0, 0.0)
    nb = int(X.shape[0]) // B
    if which == "shared_all":
        G, M = 4096, N
        index = FilterIndex([X], N, R, engine=eng)
        sf, of = index.device_filter(eng, X, "s"), index.device_filter(eng, X, "o")
        all_ids = torch.arange(N, dtype=torch.int32, device="cuda").repeat(-(-B // G), 1).contiguous()
        stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    else:
        G = M = 256

    def step(s, reg):
        r0 = (s % nb) * B
        xb = X[r0:r0 + B]
        o = _ffi.Opt(2, 2, 1e-3, .9, .999, 1e-7, 0.0, s + 1)
        if which == "shared_all":
            side = eng.sample_shared(xb, G, 1, 0, s)[1]
            cut = lambda f: (f[0][r0:r0 + B], f[1][r0:r0 + B], f[2])   # noqa: E731
            eng.train_shared_masked_fwdbwd(xb, G, M, all_ids, side, loss, s_filter=cut(sf), o_filter=cut(of), identity=True, stats=stats)
        else:
            ids, side = eng.sample_shared(xb, G, M, 0, s)
            eng.train_shared_fwdbwd(xb, G, M, ids, side, loss)
        if reg is not None:
            eng.batch_reg_fwdbwd(xb, reg, reg)
        eng.opt_step(o)

    return {"none": lambda s: step(s, None), "n3": lambda s: step(s, n3)}


def per_corruption_variants(d, X, n3):
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    N, R = d["n_ents"], d["n_rels"]
    nb = int(X.shape[0]) // B
    out = {}
    for name, reg, path in (("owner_computes", None, ""), ("dense", None, "atomic"), ("dense_n3", n3, "")):
        os.environ["AMDKGE_TRAIN_PATH"] = path   # (read once, when the loop is made)
        loop = StepLoop(new_engine(N, R), ETA, loss_functions.get("self_adversarial"), optimizers.get("adam"), reg, seed=0, dist=None)
        os.environ.pop("AMDKGE_TRAIN_PATH")
        assert loop.use_tiled == (path != "atomic")
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
    ap.add_argument("--only", nargs="+", default=None, choices=["shared_M256", "shared_all", "per_corruption"])
    ap.add_argument("--variant", default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lam", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_batch_reg: needs a GPU (no CPU fallback)")
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.latent_features.regularizers import BatchLPRegularizer

    d = make_synthetic_kg()
    X = torch.as_tensor(d["train"]).cuda()
    n3 = BatchLPRegularizer(3, a.lam)
    out = {"model": MODEL, "k": K_UNITS, "B": B, "N": d["n_ents"], "R": d["n_rels"], "lambda": a.lam, "rounds": a.rounds, "block": a.block, "groups": {}}
    for group in a.only or ["shared_M256", "shared_all", "per_corruption"]:
        variants = per_corruption_variants(d, X, n3) if group == "per_corruption" else shared_variants(d, X, group, n3)
        if a.variant:
            variants = {a.variant: variants[a.variant]}
        out["groups"][group] = time_group(variants, a.rounds, a.block, a.warmup)
        print(json.dumps({group: out["groups"][group]}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

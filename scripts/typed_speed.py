"""Development: what type-constrained negatives and evaluation cost at BASELINE configs[1] (ComplEx k=200 eta=20 self-adversarial,
B=10000 on the synthetic FB15K-237; bench.py's C2 tables and step loop).

  train   ms/step and sampler-kernel us/step of two settings, alternating repetition by repetition (median reported):
            filtered  NegativeSampling(filter=True)                 (amdkge_sample_negatives)
            typed     TypedNegatives("observed", filter=True)       (amdkge_sample_negatives_typed, the training set's sets)
          the kernel time is the sampler call alone, HIP events around `calls` back-to-back launches on the batches of an epoch
  eval    the test set, filtered, both sides: the typed pass (range lookup + amdkge_rank_lists against the relation's set, sets
          observed in train + valid + test) against the 1-vs-all pass evaluate() runs, and the mean set size per query

usage: typed_speed.py [--steps N] [--reps N] [--warmup N] [--calls N]          prints one line "TYPED_SPEED {json}" """
import argparse
import json
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()

    import numpy as np
    import torch

    sys.path.insert(0, ".")
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.datasets.filters import FilterIndex
    from ampligraph_amd.datasets.types import BoundRelationTypes
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.latent_features.negatives import BoundNegatives, BoundTypedNegatives
    from ampligraph_amd.trainer import StepLoop

    d = make_synthetic_kg("synth-fb15k237", seed=0)
    N, R, k, eta, B = d["n_ents"], d["n_rels"], 200, 20, 10000
    train = torch.as_tensor(d["train"]).cuda()
    per_epoch = max(1, train.shape[0] // B)
    batch_of = lambda s: train[(s % per_epoch) * B:(s % per_epoch) * B + B]   # noqa: E731
    rng = np.random.Generator(np.random.PCG64(0))
    lim_e, lim_r = float(np.sqrt(6.0 / (N + 2 * k))), float(np.sqrt(6.0 / (R + 2 * k)))
    ent0 = rng.uniform(-lim_e, lim_e, size=(N, 2 * k)).astype(np.float32)
    rel0 = rng.uniform(-lim_r, lim_r, size=(R, 2 * k)).astype(np.float32)

    def sets_of(eng, X):
        return BoundRelationTypes(eng, N, R, {sd: eng.relation_sets_build(X, sd, N, R) for sd in ("s", "o")})

    loops = {}
    for name in ("filtered", "typed"):
        eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
        eng.set_tables(ent0, rel0)
        loop = StepLoop(eng, eta, loss_functions.get("self_adversarial"), optimizers.get("adam"), None, seed=0, dist=None)
        loop.configure_for_data(d["train"], B)
        index = FilterIndex([train], N, R, engine=eng)
        if name == "typed":
            loop.negatives = BoundTypedNegatives(eng, train, index, "uniform", None, 8, reject=True, relation_types=sets_of(eng, train), min_size=2)
        else:
            loop.negatives = BoundNegatives(eng, train, index, "uniform", None, 8, reject=True)
        loop.reset_loss()
        for s in range(a.warmup):
            loop.step(batch_of(s), s)
        loops[name] = loop
    torch.cuda.synchronize()
    step_ms, kern_us = {n: [] for n in loops}, {n: [] for n in loops}
    nxt = a.warmup
    for _ in range(a.reps):
        for name, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(nxt, nxt + a.steps):
                loop.step(batch_of(s), s)
            torch.cuda.synchronize()
            step_ms[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for s in range(a.calls):
                loop.negatives(batch_of(s), 0, B, eta, 0, nxt + s)
            e1.record()
            torch.cuda.synchronize()
            kern_us[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
        nxt += a.steps
    done = a.warmup + a.reps * (a.steps + a.calls)
    out = {"shape": {"N": N, "R": R, "k": k, "eta": eta, "B": B}, "steps": a.steps, "reps": a.reps,
           "ms_per_step": {n: float(np.median(t)) for n, t in step_ms.items()}, "ms_min_max": {n: [min(t), max(t)] for n, t in step_ms.items()},
           "sampler_us": {n: float(np.median(t)) for n, t in kern_us.items()}, "sampler_us_min_max": {n: [min(t), max(t)] for n, t in kern_us.items()},
           "per_step": {n: {key: v / done for key, v in loop.negatives.stats().items()} for n, loop in loops.items()}}
    typed = loops["typed"].negatives
    sizes = torch.cat([c[1] - c[0] for c in (typed.s_cand, typed.o_cand)]).double()
    out["train_set_size_mean"] = float(sizes.mean())

    # ---- evaluation: the test set, filtered, both sides
    eng = loops["typed"].engine
    everything = torch.as_tensor(np.concatenate([d["train"], d["valid"], d["test"]])).cuda()
    test = torch.as_tensor(np.ascontiguousarray(d["test"])).cuda()
    fi = FilterIndex([everything], N, R, engine=eng)
    bound = sets_of(eng, everything)
    sides = (("s", _ffi.SIDE_S), ("o", _ffi.SIDE_O))

    def typed_pass():
        ranks = torch.empty(test.shape[0], 2, dtype=torch.int32, device="cuda")
        for col, (sd, side) in enumerate(sides):
            cand = (*bound.ranges(test, sd, 1, "all"), bound.max_len)
            eng.rank_lists(test, side, cand, "worst", fi.device_filter(eng, test, sd), out=ranks[:, col], out_stride=2)
        return ranks

    def all_pass():
        ranks = torch.empty(test.shape[0], 2, dtype=torch.int32, device="cuda")
        eng.rank_sides(test, [(side, fi.device_filter(eng, test, sd), ranks[:, col], 2) for col, (sd, side) in enumerate(sides)], "worst")
        return ranks

    ms = {}
    for name, fn in (("typed", typed_pass), ("all", all_pass)):
        fn()
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        ms[name] = float(np.median(t))
        out.setdefault("eval_mrr", {})[name] = float((1.0 / r.double()).mean())
    lens = torch.cat([(lambda c: c[1] - c[0])(bound.ranges(test, sd, 1, "all")) for sd, _ in sides]).double()
    out["eval"] = {"n_test": int(test.shape[0]), "ms": ms, "set_size_mean": float(lens.mean()), "set_size_max": int(lens.max()),
                   "largest_set": bound.largest_set}
    print("TYPED_SPEED " + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

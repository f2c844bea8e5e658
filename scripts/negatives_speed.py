"""Development: what compile(negatives=...) costs per train step at BASELINE configs[1] (ComplEx k=200 eta=20 self-adversarial,
B=10000 on the synthetic FB15K-237; bench.py's C2 tables and step loop), ms/step for four settings:

  none      negatives=None: the train kernels draw their own corruptions (the default path)
  trivial   the sampler with nothing to do (uniform side, no filter, no pool): one extra kernel + the override array
  filtered  filter=True
  bernoulli filter=True, side="bernoulli"

usage: negatives_speed.py [--base DIR]
The measurement runs in a child process per tree (this file with --worker, the tree as its working directory, like
scripts/session_speed.py imports the package from "."), each under its own `timeout`; the first child that fails ends the run.
--base DIR: a checkout of the commit to compare with, built (its own library): its default step -- setting "none", the only one an
older tree knows -- is measured before and after this tree's four settings, in the same session on the same device.  Inside a
worker the settings alternate, repetition by repetition, and the median repetition is reported."""
import argparse
import json
import os
import subprocess
import sys
import time

SETTINGS = ("none", "trivial", "filtered", "bernoulli")


def worker(settings, steps, reps, warmup):
    import numpy as np
    import torch

    sys.path.insert(0, ".")
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers
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
    loops = {}
    for name in settings:
        eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
        eng.set_tables(ent0, rel0)
        loop = StepLoop(eng, eta, loss_functions.get("self_adversarial"), optimizers.get("adam"), None, seed=0, dist=None)
        loop.configure_for_data(d["train"], B)
        if name != "none":
            from ampligraph_amd.datasets.filters import FilterIndex
            from ampligraph_amd.latent_features.negatives import BoundNegatives

            index = FilterIndex([train], N, R, engine=eng) if name != "trivial" else None
            loop.negatives = BoundNegatives(eng, train, index, "bernoulli" if name == "bernoulli" else "uniform", None, 8, reject=name != "trivial")
        loop.reset_loss()
        for s in range(warmup):
            loop.step(batch_of(s), s)
        loops[name] = loop
    torch.cuda.synchronize()
    times = {name: [] for name in settings}
    nxt = warmup
    for _ in range(reps):
        for name, loop in loops.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(nxt, nxt + steps):
                loop.step(batch_of(s), s)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
        nxt += steps
    out = {"ms_per_step": {n: float(np.median(t)) for n, t in times.items()}, "ms_min_max": {n: [min(t), max(t)] for n, t in times.items()},
           "steps": steps, "reps": reps, "loss": {n: loops[n].mean_batch_loss() for n in settings}}
    for name, loop in loops.items():
        if getattr(loop, "negatives", None) is not None:   # (a --base tree may be older than the attribute)
            st = loop.negatives.stats()
            out.setdefault("per_step", {})[name] = {key: v / (warmup + reps * steps) for key, v in st.items()}
    print("NEGATIVES_SPEED " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", default=None, help="a built checkout of the commit to compare with")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--settings", default=",".join(SETTINGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--limit", type=int, default=300, help="seconds a child may take")
    a = ap.parse_args()
    if a.worker:
        return worker(a.settings.split(","), a.steps, a.reps, a.warmup)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = [("this tree", here, a.settings)]
    if a.base:
        runs = [("base (before)", a.base, "none")] + runs + [("base (after)", a.base, "none")]
    for label, tree, settings in runs:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--worker", "--settings", settings,
               "--steps", str(a.steps), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("NEGATIVES_SPEED ")]
        if r.returncode != 0 or not line:
            print(f"{label}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            return r.returncode or 1
        res = json.loads(line[0][len("NEGATIVES_SPEED "):])
        print(f"{label} ({tree}):")
        for name, ms in res["ms_per_step"].items():
            lo, hi = res["ms_min_max"][name]
            extra = "".join(f"  {key}/step {v:.1f}" for key, v in res.get("per_step", {}).get(name, {}).items())
            print(f"  {name:10s} {ms:.4f} ms/step  (repetitions {lo:.4f} .. {hi:.4f})  mean batch loss {res['loss'][name]:.4f}{extra}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X.

Metric (BASELINE.json): training triples/s INCLUDING negatives, ComplEx k=200, eta=20,
self-adversarial NLL, Adam, on an FB15K-237-shaped synthetic graph (configs[1]); batch 10 000
positives per GPU per step (the reference docstring's batch, ScoringBasedEmbeddingModel.py:66).
One "step" = one pass of the hot path over one batch = the product's StepLoop.step: at N=1 the
owner-computes pair (kge_train_tiled.hip: fused lookup/sampling/score/loss/backward + staging kernel,
then the per-tile LDS accumulation kernel that also applies Adam to both tables); at N>1 the same pair
in its gradient-only form + the data-parallel merge over RCCL/xGMI (reduce-scatter by all_to_all, sharded
optimizer sweep, all_to_all of the updated parameter slices; AMDKGE_DP_MERGE=allreduce for one all-reduce).

Contract: `python bench.py --gpus N --steps K --warmup W`.  For N>1 the driver launches it under torch.distributed.run (one
rank per GPU); started WITHOUT a launcher (`python bench.py --gpus N`, WORLD_SIZE unset) the script launches its own N ranks
the same way and fails loudly when the node has fewer than N GPUs (AMDKGE_BENCH_BACKEND=gloo: development, N ranks on the GPUs
there are).  Rank 0 prints ONE JSON line.  The timed region contains nothing but the K calls of the step (no event records),
bracketed by barrier + synchronize (max over ranks).

A plain run does only what the headline needs: set up, W warm-up steps, ONE timed region of exactly K steps, the line.
`--full` adds everything else, as the default command did before it existed: the timed region repeated --reps times (default 5;
`ms_per_step` / `value` are then the MEDIAN repetition), the per-phase HIP events of a separate, untimed pass of the same steps,
`roofline` (the train-step kernel pair, HBM-bound, algorithmic bytes 2*(3+eta)*4K per positive; duration = HIP
events on the launch stream around the pair, i.e. the sum of the two kernels' durations + one launch gap), `cpu_baseline`
(oracle/ref_cpu.py, the op-for-op torch-CPU port, on a bounded sample), `eval` (filtered ranks/s of evaluate() on the 20 438
synthetic test triples, N=1 only), the drop-in class's fit() / evaluate() and the other presets under `extra_configs`.

`--dump-outputs DIR` writes, right after the timed steps, what a caller of the timed path holds after its last step (see
dump_outputs) as DIR/<name>.npy.  The inputs depend on the arguments only (seeded graph, tables and negatives).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


# BASELINE.json `configs`, in its order (C1 = configs[0] ... C5 = configs[4]).  C2 is the configuration the metric is quoted on
# and the default workload; the others are selected with --config.  C4 / C5 row-shard the entity table when N > 1.
PRESETS = {
    "C1": dict(model="TransE", k=50, eta=5, loss="pairwise", dataset="synth-fb15k237", batch=10000, parallelism="replicated"),
    "C2": dict(model="ComplEx", k=200, eta=20, loss="self_adversarial", dataset="synth-fb15k237", batch=10000, parallelism="replicated"),
    "C3": dict(model="DistMult", k=400, eta=30, loss="self_adversarial", dataset="synth-wn18rr", batch=10000, parallelism="replicated"),
    "C4": dict(model="ComplEx", k=200, eta=20, loss="self_adversarial", dataset="synth-yago310", batch=8192, parallelism="sharded-local"),
    # 50 M entities / 500 M triples over 8 GPUs = 6.25 M rows per GPU (weak scaling: the shard size is per GPU), triples from
    # the on-device counter RNG; touched-rows Adam (north_star: "sparse Adam"), see --optimizer-mode
    "C5": dict(model="RotatE", k=1000, eta=64, loss="self_adversarial", dataset="synth-50M", batch=65536, parallelism="sharded-local",
               optimizer_mode="lazy"),
}
SYNTH_STREAM = {"synth-50M": dict(ents_per_gpu=6_250_000, n_rels=1000)}   # datasets that exist only as a device-side stream


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=280)
    ap.add_argument("--warmup", type=int, default=28)
    ap.add_argument("--config", default=None, choices=sorted(PRESETS), help="a BASELINE.json configuration; explicit flags override it")
    ap.add_argument("--batch", type=int, default=None, help="positives per GPU per step")
    ap.add_argument("--model", default=None)
    ap.add_argument("--k", type=int, default=None)
    ap.add_argument("--eta", type=int, default=None)
    ap.add_argument("--loss", default=None)
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--ents-per-gpu", type=int, default=None, help="synth-50M only: rows of the entity table per GPU (cut-down runs)")
    ap.add_argument("--popularity", default="uniform", choices=["uniform", "zipf"],
                    help="entity/relation popularity of the synthetic graph (SURVEY.md 8d: uniform primary, zipf secondary)")
    ap.add_argument("--optimizer-mode", default=None, choices=["dense", "lazy"],
                    help="dense = the reference's Keras-legacy behaviour (every row every step); lazy = touched rows only "
                         "(amdkge_opt.lazy, a documented deviation)")
    ap.add_argument("--deterministic", action="store_true", help="AMDKGE_TILED_DETERMINISTIC: bitwise reproducible tables (sorted tile "
                    "accumulation, staged relation gradient); reports its cost")
    ap.add_argument("--skew-mode", default="auto", choices=["auto", "none", "atomic", "hot"],
                    help="development: how the positives' own rows of hot entities are handled (auto = configure_for_data decides; none = all "
                         "staged; atomic = AMDKGE_TILED_POS_ATOMIC; hot = replica rows for the hot entities only)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline: repeated timed regions, per-phase events, roofline, "
                    "evaluation, drop-in calls, CPU baselines, the other presets (a plain run times ONE region of --steps steps)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write the timed path's outputs after its last timed step as "
                    "DIR/<name>.npy (fp32 / fp64, at most 64 MB in all)")
    ap.add_argument("--reps", type=int, default=None, help="repetitions of the timed K-step region; the median is reported (min / max beside "
                    "it).  Default: 1, with --full 5")
    ap.add_argument("--phase-steps", type=int, default=32, help="--full: steps of the separate, untimed pass that records the per-phase HIP events")
    ap.add_argument("--also", default=None, help="--full: comma-separated presets run after the main one in the same process (N=1 only); their "
                    "lines go under `extra_configs`.  Default: C1, C3, C4, C5 beside the default C2 run; 'none' = off")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-eval", action="store_true")
    ap.add_argument("--dropin", action="store_true", help="--full: also time whole fit() / evaluate() calls of the drop-in class (always on for the C2 preset)")
    ap.add_argument("--trained-eval", action="store_true", help="--full: also time evaluate() on trained-like tables (always on for the C2 preset)")
    ap.add_argument("--cpu-steps", type=int, default=8)
    ap.add_argument("--parallelism", default=None, choices=["replicated", "sharded-local", "sharded-global", "columns"],
                    help="N>1: replicated tables + gradient merge (right for tables that fit one GPU), the "
                         "row-sharded entity table of ampligraph_amd/sharded.py with shard-local / global negatives, or COLUMN-sharded "
                         "tables (ampligraph_amd/colsharded.py: every rank holds k / N units of every row and processes the whole "
                         "global batch; one all-reduce of the partial scores per step)")
    ap.add_argument("--cols-of", type=int, default=None,
                    help="with --parallelism columns on ONE GPU: measure the work of ONE rank of a W-rank column-sharded run -- a k / W "
                         "slice, the global batch of W x --batch positives, the score all-reduce through whatever process group exists "
                         "(AMDKGE_BENCH_FORCE_DIST=1: a one-rank RCCL group)")
    args = ap.parse_args()
    preset = dict(PRESETS[args.config or "C2"])
    for key, val in preset.items():
        if getattr(args, key, None) is None:
            setattr(args, key, val)
    if args.optimizer_mode is None:
        args.optimizer_mode = "dense"
    args.preset = args.config or ("C2" if all(getattr(args, k_) == v_ for k_, v_ in PRESETS["C2"].items()) else None)
    if not args.full and ((args.also or "none") != "none" or args.dropin or args.trained_eval):
        ap.error("--also, --dropin and --trained-eval are measurements beside the headline: they need --full")
    if args.reps is None:
        args.reps = 5 if args.full else 1
    if args.also is None:   # the full run also reports C1, C3, C4 and one GPU's C5 shard (VERDICT r3 #8, r5 #3 / missing #3)
        args.also = "C1,C3,C4,C5" if (args.full and args.preset == "C2" and args.gpus == 1 and args.popularity == "uniform"
                                   and not args.deterministic and args.optimizer_mode == "dense") else "none"
    return args


def preset_args(base, name):
    """argparse namespace of preset `name` with the run-control flags (steps, warmup, reps, ...) of `base`."""
    import copy

    a = copy.copy(base)
    for key, val in PRESETS[name].items():
        setattr(a, key, val)
    a.config = a.preset = name
    a.optimizer_mode = PRESETS[name].get("optimizer_mode", "dense")
    a.also = "none"
    a.dump_outputs = None   # the outputs written are the headline configuration's
    if name in ("C1", "C4") and base.preset != name:   # riding along in another config's line: the CPU legs (C4: a 123 k-row dense Adam on the host) are left out
        a.no_cpu_baseline = True
    if name == "C5" and base.preset != "C5":
        # one GPU's shard of configs[4] riding along (RotatE k = 1000, eta = 64, 6.25 M rows = 50 GB table, 200 GB resident, B = 65 536;
        # a step is 40 - 66 ms): a handful of steps, tables drawn on the device, no evaluation (2 N K per rank on 6.25 M rows), no CPU leg
        a.steps, a.warmup, a.reps, a.phase_steps = min(int(base.steps), 4), 1, 2, 2
        a.no_cpu_baseline = a.no_eval = True
    return a


def cpu_baseline(args, data, ent0, rel0):
    """The reference-equivalent CPU path (oracle/ref_cpu.py) timed on this box's host cores: a bounded
    sample of the SAME workload (first `cpu_steps`+1 batches, first one untimed)."""
    from oracle import ref_cpu

    cores = os.cpu_count() or 1
    X = torch.as_tensor(data["train"].astype(np.int64))
    B = args.batch
    # torch's intra-op pool does not scale to hundreds of threads on this op mix: probe a few pool sizes
    # with one step each and keep the fastest (threads actually used are reported as `cores`)
    best = None
    for th in sorted({min(cores, t) for t in (8, 16, 32, 64, cores)}):
        torch.set_num_threads(th)
        tr = ref_cpu.RefCpuTrainer(args.model, ent0, rel0, args.eta, args.loss, 1e-3, data["n_rels"])
        tr.step(X[:B])  # warm-up (allocator, thread pool)
        t0 = time.perf_counter()
        tr.step(X[B:2 * B])
        d1 = time.perf_counter() - t0
        if best is None or d1 < best[0]:
            best = (d1, th)
    torch.set_num_threads(best[1])
    tr = ref_cpu.RefCpuTrainer(args.model, ent0, rel0, args.eta, args.loss, 1e-3, data["n_rels"])
    tr.step(X[:B])
    t0 = time.perf_counter()
    for s in range(1, args.cpu_steps + 1):
        tr.step(X[s * B:(s + 1) * B])
    dt = time.perf_counter() - t0
    return {"value": args.cpu_steps * B * (1 + args.eta) / dt, "unit": "triples/s", "cores": torch.get_num_threads(),
            "kind": "port", "host_cores": cores,
            "sample": f"{args.cpu_steps} train steps of B={B} (after 1 warm-up step), same tables and triples; "
                      "oracle/ref_cpu.py = op-for-op torch-CPU restatement of the reference TF graph "
                      "(TensorFlow itself is not installable here)"}


def cpu_eval_baseline(args, data, ent, rel, n_sample=1024, batch=256):
    """The evaluation half of the metric on the host cores: oracle/ref_cpu.rank_batch (the reference's evaluate() structure --
    per-batch 1-vs-all scores as ONE matmul, i.e. kinder than the reference's (n, m, K) broadcast, quantise, compare-count, the
    per-triple filter subtraction of AbstractScoringLayer.py:260-307) on a bounded sample of the same test split, both sides,
    filtered.  The filter sets of the sample are built beforehand and not timed (nor is the device-side index build in `eval`)."""
    from oracle import kge_oracle as O
    from oracle import ref_cpu

    if args.model == "RotatE":
        return None   # (rank_batch has no RotatE form)
    test = data["test"][:n_sample]
    fs, fo = O.filter_sets(test, [data["train"], data["valid"], data["test"]])
    fs = [torch.as_tensor(f, dtype=torch.int64) for f in fs]
    fo = [torch.as_tensor(f, dtype=torch.int64) for f in fo]
    E, Rl = torch.as_tensor(ent), torch.as_tensor(rel)
    best = None
    for th in sorted({min(os.cpu_count() or 1, t) for t in (8, 32, 64)}):
        torch.set_num_threads(th)
        ref_cpu.rank_batch(args.model, E, Rl, test[:batch], fs[:batch], fo[:batch], data["n_rels"])
        t0 = time.perf_counter()
        ref_cpu.rank_batch(args.model, E, Rl, test[:batch], fs[:batch], fo[:batch], data["n_rels"])
        d1 = time.perf_counter() - t0
        if best is None or d1 < best[0]:
            best = (d1, th)
    torch.set_num_threads(best[1])
    t0 = time.perf_counter()
    for b0 in range(0, len(test), batch):
        ref_cpu.rank_batch(args.model, E, Rl, test[b0:b0 + batch], fs[b0:b0 + batch], fo[b0:b0 + batch], data["n_rels"])
    dt = time.perf_counter() - t0
    return {"value": 2 * len(test) / dt, "unit": "filtered ranks/s", "cores": best[1], "kind": "port",
            "sample": f"{len(test)} test triples x 2 sides in batches of {batch} against all {data['n_ents']} entities (oracle/ref_cpu.rank_batch: "
                      "matmul 1-vs-all + quantise + compare-count + per-triple filter loop); filter sets prebuilt, untimed"}


def eval_bench(eng, data, rank, triples=None, filter_sets=None):
    """Filtered evaluate() of the synthetic test split (or of `triples`), both sides: ranks/s (BASELINE.json metric, part 2)."""
    from ampligraph_amd import _ffi
    from ampligraph_amd.datasets.filters import FilterIndex

    test = data["test"] if triples is None else triples
    if filter_sets is not None:
        data = dict(data, train=filter_sets[0], valid=filter_sets[0][:0], test=test)
    n = test.shape[0]
    dev = eng.device
    Xd = torch.as_tensor(test).to(dev)
    # first-use costs, untimed: the process's first large pageable H2D copy alone takes ~20 ms
    FilterIndex([data["train"], data["valid"], test], data["n_ents"], data["n_rels"], engine=eng).device_filter(eng, Xd, "s")
    torch.cuda.synchronize()
    # the filter index (train + valid + test: 310 k triples at C2): upload of the id triples, device build (amdkge_filter_build:
    # keys, radix sort, scan, scatter) and the per-triple range lookup (amdkge_filter_ranges) -- what evaluate() does
    t0 = time.perf_counter()
    fi = FilterIndex([data["train"], data["valid"], test], data["n_ents"], data["n_rels"], engine=eng)
    fs = fi.device_filter(eng, Xd, "s")
    fo = fi.device_filter(eng, Xd, "o")
    torch.cuda.synchronize()
    index_ms = (time.perf_counter() - t0) * 1e3
    ranks = torch.empty(n, 2, dtype=torch.int32, device=dev)

    def run():   # (what models.evaluate does: both sides in flight, each on its own stream)
        if os.environ.get("AMDKGE_BENCH_EVAL_SERIAL", "0") == "1":
            eng.rank_side(Xd, _ffi.SIDE_S, "worst", fs, out=ranks[:, 0], out_stride=2)
            eng.rank_side(Xd, _ffi.SIDE_O, "worst", fo, out=ranks[:, 1], out_stride=2)
        else:
            eng.rank_sides(Xd, [(_ffi.SIDE_S, fs, ranks[:, 0], 2), (_ffi.SIDE_O, fo, ranks[:, 1], 2)], "worst")

    # Both paths (the default one here, the exact kernels below) are timed the same way: two untimed calls, then `reps` back to back.
    # The filter index above is host work during which the GPU idles and its clocks fall; with ONE warm-up call the path timed FIRST
    # paid for the ramp -- round 4 read that as "the probe costs an untrained TransE table 8 %": the kernel trace shows the first
    # repetitions after the pause 5.85 / 5.60 ms and the later ones 5.3 ms whichever path they belong to
    # (profiles/r05e_transe_eval_trace.txt).
    def timed(reps=5):
        """-> the repetitions' durations (each one whole evaluate() of both sides, synchronised)"""
        run()
        run()
        torch.cuda.synchronize()
        out_s = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            out_s.append(time.perf_counter() - t0)
        return out_s

    reps_first = timed()
    dt = float(np.mean(reps_first))
    r = ranks.cpu().numpy()
    scr = eng.screen_stats()   # int8 screening pass (contraction models) / exact early exit (distance models): pairs the exact chain had to recheck (last side)
    dist_model = eng.scoring_type in ("TransE", "RotatE")
    # the same evaluation through the exact fp32 matrix-core kernel alone (round 2's path): ranks must be identical, time beside it
    exact = None
    if scr is not None:
        try:
            _ffi.check(eng.lib.amdkge_set_rank_kernel(1 if dist_model else 3))
            dte = float(np.median(timed()))
            exact = {"ms": dte * 1e3, "ranks_per_s": 2 * n / dte, "ranks_identical_to_screened": bool(np.array_equal(ranks.cpu().numpy(), r)),
                     "kernel": ("the plain tile kernel (rank_count_kernel / rank_rot_kernel): every pair's full chain" if dist_model else
                                "rank_count_mfma_pipe_kernel (v_mfma_f32_32x32x2_f32) for every pair")}
        finally:
            eng.lib.amdkge_set_rank_kernel(0)
        # ... and the default path once more, behind the exact one.  Reported: the MEDIAN of all ten timed repetitions;
        # the two passes' means stand beside it (round 5 reported the faster mean: an 11 % spread on the driver's C3 line)
        reps_again = timed()
        dt_first, dt_again = float(np.mean(reps_first)), float(np.mean(reps_again))
        dt = float(np.median(reps_first + reps_again))
    else:
        dt_first = dt_again = dt
        dt = float(np.median(reps_first))
    flops = 2.0 * data["n_ents"] * eng.K * n * 2
    # the evaluation half of BASELINE.json's metric on the footing of the training half: SURVEY.md 8(d) prices a rank at 2 N K flop
    # against the fp32 matrix peak (157.3 TFLOP/s; the distance models run the same count of fp32 VALU operations against the same
    # vector peak).  `achieved` is the EXACT fp32 kernel's rate over the whole evaluate() (prep, counts, filter pass, compose) -- the
    # screened / early-exit default path decides most pairs without that work, so its equivalent rate stands beside it, not in frac.
    peak_tf = 157.3
    exact_tf = (flops / (exact["ms"] * 1e-3) / 1e12) if exact else None
    util, util_src = None, None
    if not dist_model:
        for cand in ("r06_pmc_screen.json", "r05_pmc_screen.json", "r04_pmc_screen.json", "r03_pmc_screen.json"):
            f = os.path.join(ROOT, "profiles", cand)
            if os.path.exists(f):
                try:
                    util = json.load(open(f)).get("mfma_util")
                    util_src = f"replayed from profiles/{cand} (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES pass of rank_screen_kernel at the C2 shape; not measured in this run)"
                except Exception:
                    util = None
                break
    roof = {"bound": "valu" if dist_model else "mfma",
            "kernel": ("rank_count_kernel / rank_rot_kernel (fp32 VALU chains)" if dist_model else "rank_count_mfma_pipe_kernel (v_mfma_f32_32x32x2_f32)"),
            "flops_per_rank": 2.0 * data["n_ents"] * eng.K, "achieved": exact_tf, "achieved_tf": exact_tf, "peak": peak_tf, "unit": "TFLOP/s",
            "frac": (exact_tf / peak_tf) if exact_tf else None,
            "achieved_is": "the exact fp32 kernel path timed over the whole evaluate() of both sides (exact_fp32_kernel_alone.ms)",
            "screened_equivalent_tf": flops / dt / 1e12, "int8_mfma_util": util, "int8_mfma_util_source": util_src}
    return {"ranks_per_s": 2 * n / dt, "ms": dt * 1e3, "ms_is": "median of all timed repetitions of the default path (5 before + 5 after the exact-kernel pass)",
            "ms_mean_before_and_after_the_exact_path": [dt_first * 1e3, dt_again * 1e3],
            "n_test": int(n), "sides": 2, "filtered": True,
            # what the reference's evaluate() includes (its per-batch pandas filter look-ups, graph_data_loader.py:287-350,382-439):
            # the device build of the filter index + the range look-ups of both sides, once per evaluate() call
            "ranks_per_s_incl_filter_build": 2 * n / (dt + index_ms * 1e-3), "roofline": roof,
            "filter_index_ms": index_ms, "filter_index": "built on the device (upload + amdkge_filter_build + amdkge_filter_ranges, both sides)",
            # 2 N K flop per rank over the whole evaluation: what an fp32 contraction of every (query, entity) pair would have had to
            # sustain (fp32 matrix peak 157.3 TFLOP/s) -- with the screening pass most pairs are decided in int8, so this is an
            # EQUIVALENT rate, not fp32 work done
            "equivalent_fp32_tflops": flops / dt / 1e12,
            "screening": (None if scr is None else {"rechecked_pairs_per_side": scr[0], "fraction": scr[0] / float(n * data["n_ents"]),
                                                    "fell_back_to_exact_kernel": scr[1],
                                                    "note": ("exact early exit: a pair is dropped once its monotone fp32 partial sum quantises below the positive's "
                                                             "score; tiles with few undecided pairs hand them to a list whose chains are recomputed in full: counts "
                                                             "bit-identical to the plain kernels" if dist_model else
                                                             "int8 matrix-core pass decides the comparisons a rigorous error bound allows; the "
                                                             "rest are recomputed with the exact fp32 chain: counts bit-identical to the fp32 kernels")}),
            "exact_fp32_kernel_alone": exact,
            "mrr_untrained_tables": float(np.mean(1.0 / r)), "note": "tables as left by the timed training steps"}


def dropin_bench(args, data, ms_per_step, eval_ms):
    """The drop-in CLASS on the clock: what a user of the reference calls is
    ScoringBasedEmbeddingModel.fit() / evaluate() (/root/reference/ampligraph/latent_features/models/ScoringBasedEmbeddingModel.py:832-876,
    1516-1692), not StepLoop.step / rank_sides.  `fit_epoch_ms`: fit(X, batch_size=B, epochs=5) on the same synthetic graph (integer ids:
    the label -> id mapping runs, string handling is skipped), epochs 2-4 timed between on_epoch_end callbacks (each epoch ends with the
    read-back of its mean loss, i.e. synchronised).  `evaluate_call_ms`: ONE whole evaluate(test, use_filter={train, valid, test},
    corrupt_side="s,o") -- id mapping of the test set and of the 310 k filter triples, device build of the filter index, both sides'
    ranks, D2H -- in a warm process with the filter cache emptied; beside it the call that finds its filter index cached, which is what
    validation inside fit() and repeated evaluate() calls pay."""
    from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel, optimizers

    class Clock:
        def __init__(self):
            self.t = []

        def on_train_begin(self):
            self.t.append(time.perf_counter())

        def on_epoch_end(self, epoch, logs=None):
            torch.cuda.synchronize()
            self.t.append(time.perf_counter())

    B = args.batch
    m = ScoringBasedEmbeddingModel(eta=args.eta, k=args.k, scoring_type=args.model, seed=0)
    m.compile(optimizer=optimizers.get("adam", {"learning_rate": 1e-3}), loss=args.loss)
    clk = Clock()
    t0 = time.perf_counter()
    m.fit(data["train"], batch_size=B, epochs=5, verbose=False, callbacks=[clk])
    fit_total = time.perf_counter() - t0
    ep = np.diff(clk.t) * 1e3                      # ms per epoch, epochs 1..5
    steps = -(-data["train"].shape[0] // B)
    fit_epoch_ms = float(np.mean(ep[1:4]))
    flt = {"train": data["train"], "valid": data["valid"], "test": data["test"]}

    def one_call():
        t1 = time.perf_counter()
        r = m.evaluate(data["test"], use_filter=flt, corrupt_side="s,o", verbose=False)
        return (time.perf_counter() - t1) * 1e3, r

    first_ms, ranks = one_call()                   # first use in this model: library warm (eval_bench ran), caches cold
    cold = []
    for _ in range(3):
        m._filter_cache = (None, None)
        cold.append(one_call()[0])
    cached = [one_call()[0] for _ in range(3)]
    ev_ms, ev_cached = float(np.median(cold)), float(np.median(cached))
    return {"what": "ScoringBasedEmbeddingModel.fit / evaluate of the drop-in class, whole calls (host indexing, per-epoch read-back, filter build, D2H included)",
            "fit_epoch_ms": fit_epoch_ms, "fit_epoch_ms_each": [float(x) for x in ep], "fit_call_s_5_epochs": fit_total,
            "steps_per_epoch": int(steps), "batch_size": int(B),
            "fit_epoch_over_28_steps": fit_epoch_ms / (28.0 * ms_per_step),
            "fit_epoch_over_its_own_steps": fit_epoch_ms / ((data["train"].shape[0] / float(B)) * ms_per_step),
            "fit_triples_per_s": data["train"].shape[0] * (1 + args.eta) / (fit_epoch_ms * 1e-3),
            "evaluate_call_ms": ev_ms, "evaluate_call_ms_each": [float(x) for x in cold], "evaluate_first_call_ms": first_ms,
            "evaluate_call_cached_filter_ms": ev_cached, "evaluate_call_over_eval_ms": (ev_ms / eval_ms) if eval_ms else None,
            "evaluate_cached_over_eval_ms": (ev_cached / eval_ms) if eval_ms else None,
            "evaluate_ranks_per_s": 2 * data["test"].shape[0] / (ev_ms * 1e-3), "n_test": int(data["test"].shape[0]),
            "mrr": float(np.mean(1.0 / np.asarray(ranks, dtype=np.float64)))}


def plant_fitted_triples(eng, data, model, k, noise_rel=0.5, seed=1):
    """Tables in the state a FITTED distance model leaves them in, without training one: n triples (s from the first half of the
    entities, distinct o from the second half, random p) whose object row is set to the model's own prediction for it -- s + p
    (TransE.py:51-53) resp. s o r (RotatE.py:96-101) -- plus N(0, (noise_rel x the table's std)^2).  The synthetic graphs are
    uniform-random (nothing to learn: MRR stays at chance however long one trains), so this is how the evaluation kernels are
    shown the regime they meet in practice -- positives that score near the top.  Returns the (n, 3) int32 triples."""
    import math

    rng = np.random.default_rng(seed)
    N, R = data["n_ents"], data["n_rels"]
    half = N // 2
    n = min(half, N - half, data["test"].shape[0])
    s_id, p_id = rng.integers(0, half, n), rng.integers(0, R, n)
    o_id = half + rng.permutation(N - half)[:n]
    ent, rel = eng.get_tables()
    s, p = ent[s_id], rel[p_id]
    if model == "TransE":
        pred = s + p
    else:
        div = math.sqrt(6.0 / (2 * k * R)) / math.pi   # RotatE.py:57-60 (embedding_range / pi)
        phi = p[:, :k].astype(np.float64) / div
        sr, si = s[:, :k].astype(np.float64), s[:, k:].astype(np.float64)
        pred = np.concatenate([sr * np.cos(phi) - si * np.sin(phi), sr * np.sin(phi) + si * np.cos(phi)], 1)
    ent[o_id] = (pred + rng.normal(size=pred.shape) * noise_rel * float(ent.std())).astype(np.float32)
    eng.set_tables(ent, rel)
    return np.stack([s_id, p_id, o_id], 1).astype(np.int32)


DUMP_TABLE_BYTES = {"entity": 48 << 20, "relation": 8 << 20}   # --dump-outputs: under 64 MB in all, row ids included


def dump_outputs(path, eng, n_rows, loss_mean):
    """--dump-outputs: what a caller of the timed path (the step loop) holds after its last timed step -- both trained tables
    in the dense [n, K] fp32 layout get_tables() returns (this rank's rows: its shard when the entity table is row-sharded, its
    column slice when column-sharded) and the mean batch loss since the warm-up began (fp64, what fit() reports).  A table
    larger than its share of the budget is written as a fixed, seeded sample of rows; <table>_rows.npy holds the row ids (fp64)."""
    os.makedirs(path, exist_ok=True)
    for name, table, n in (("entity", eng.ent, n_rows), ("relation", eng.rel, eng.n_rels)):
        per_row = 4 * eng.K + 8
        if n * per_row <= DUMP_TABLE_BYTES[name]:
            ids = np.arange(n, dtype=np.int64)
            rows = eng.unpack(table[:n])
        else:
            ids = np.sort(np.random.default_rng(0).choice(n, DUMP_TABLE_BYTES[name] // per_row, replace=False))
            rows = eng.unpack(table.index_select(0, torch.as_tensor(ids, device=table.device)))
        np.save(os.path.join(path, f"{name}_table.npy"), rows.cpu().numpy().astype(np.float32, copy=False))
        np.save(os.path.join(path, f"{name}_table_rows.npy"), ids.astype(np.float64))
    np.save(os.path.join(path, "mean_batch_loss.npy"), np.array([loss_mean], dtype=np.float64))


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N ranks of this script under torch.distributed.run (what the
    driver's own command line does) and pass their output through.  One rank per GPU: a node with fewer than N GPUs is an
    error, not a silent one-GPU run (AMDKGE_BENCH_BACKEND=gloo lifts that for development: ranks share the GPUs there are)."""
    import socket
    import subprocess

    backend = os.environ.get("AMDKGE_BENCH_BACKEND", "nccl")
    have = torch.cuda.device_count()
    if backend == "nccl" and have < args.gpus:
        raise SystemExit(f"bench.py --gpus {args.gpus}: this node has {have} GPU(s); one rank per GPU is required "
                         "(AMDKGE_BENCH_BACKEND=gloo runs several ranks per GPU for development)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


class Ctx:
    """launch context of this process: ranks, backend, the torch.distributed module (None: no process group)"""
    world = 1
    rank = 0
    backend = None
    dist = None
    multi = False       # the multi-rank code paths are taken (world > 1, or a forced process group of one rank)
    forced = False
    rccl = None


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args)
    ctx = Ctx()
    ctx.world = world = int(os.environ.get("WORLD_SIZE", "1"))
    ctx.rank = rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # AMDKGE_BENCH_BACKEND=gloo (development): several ranks on ONE GPU, collectives through the host -- exercises the
    # multi-rank code path of this script on a single-GPU box; the driver's runs use nccl (= RCCL over xGMI)
    ctx.backend = backend = os.environ.get("AMDKGE_BENCH_BACKEND", "nccl")
    # AMDKGE_BENCH_FORCE_DIST=1 (development): a process group of ONE rank and the multi-rank code paths anyway
    # (gradient-only kernels, merge schedules, row exchange) -- every collective really goes through RCCL on the one GPU
    ctx.forced = world == 1 and os.environ.get("AMDKGE_BENCH_FORCE_DIST", "0") == "1"
    ctx.multi = world > 1 or ctx.forced
    if backend == "nccl" and torch.cuda.device_count() <= local_rank:
        raise SystemExit(f"rank {rank}: no GPU for LOCAL_RANK={local_rank} ({torch.cuda.device_count()} visible); one rank per GPU")
    dev_index = local_rank % max(1, torch.cuda.device_count()) if backend != "nccl" else local_rank
    torch.cuda.set_device(dev_index)
    if ctx.multi:
        import torch.distributed as dist

        if ctx.forced:
            import socket

            os.environ["AMDKGE_FORCE_DIST"] = "1"   # trainer.StepLoop: the multi-rank step with world size 1
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                with socket.socket() as sk:
                    sk.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{dev_index}"))
            try:
                ctx.rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as e:   # noqa: BLE001 -- reported, not fatal
                ctx.rccl = f"unknown ({e})"
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        ctx.dist = dist
    out = run_config(args, ctx)
    if rank == 0:
        extra = {}
        for name in [n for n in args.also.split(",") if n and n != "none"]:
            if ctx.multi:
                break
            torch.cuda.empty_cache()
            t_extra = time.perf_counter()
            if name == "C5":   # configs[4] on the driver's clock: ONE GPU's shard, the reference's dense Adam and touched rows
                shard = {"what": "ONE GPU's shard of BASELINE configs[4] (50 M entities over 8 GPUs = 6.25 M rows per GPU, weak scaling), single-GPU "
                                 "step on it: no exchange of remote rows in this measurement"}
                for mode in ("dense", "lazy"):
                    pa = preset_args(args, "C5")
                    pa.optimizer_mode = mode
                    t_mode = time.perf_counter()
                    try:
                        e = run_config(pa, ctx)
                        shard[mode] = {k_: e[k_] for k_ in ("metric", "value", "unit", "steps", "warmup", "repetitions", "ms_per_step", "ms_per_step_min",
                                                           "ms_per_step_max", "dtype", "config", "phases_ms", "roofline") if k_ in e}
                        shard[mode]["wall_s"] = round(time.perf_counter() - t_mode, 1)
                    except Exception as exc:   # noqa: BLE001 -- reported in the line
                        shard[mode] = {"error": f"{type(exc).__name__}: {exc}"}
                    del pa
                    e = None
                    import gc

                    gc.collect()
                    torch.cuda.empty_cache()
                shard["wall_s"] = round(time.perf_counter() - t_extra, 1)
                extra["C5_one_gpu_shard"] = shard
                continue
            try:   # an extra configuration must never cost the headline line
                e = run_config(preset_args(args, name), ctx)
            except Exception as exc:   # noqa: BLE001 -- reported in the line
                extra[name] = {"error": f"{type(exc).__name__}: {exc}"}
                continue
            # the same fields, without repeating what does not change between configs
            extra[name] = {k_: e[k_] for k_ in ("metric", "value", "unit", "ms_per_step", "ms_per_step_min", "ms_per_step_max", "dtype",
                                                "config", "roofline", "eval", "eval_trained_like", "cpu_baseline", "dropin") if k_ in e}
            extra[name]["wall_s"] = round(time.perf_counter() - t_extra, 1)
        # ... and ONE RANK's share of an 8-way column-sharded step of the headline workload (what decides whether the
        # north_star's 8-GPU figure is reachable is a per-rank compute time, and that is measurable on one GPU): a k / 8 slice, the
        # global batch of 8 x 10 000 positives, no process group here (the 6.7 MB score all-reduce is skipped and says so)
        if extra and not ctx.multi and args.preset == "C2":
            import copy

            ca = copy.copy(args)
            ca.parallelism, ca.cols_of, ca.no_eval, ca.no_cpu_baseline, ca.also, ca.dump_outputs = "columns", 8, True, True, "none", None
            t_extra = time.perf_counter()
            try:
                torch.cuda.empty_cache()
                e = run_config(ca, ctx)
                extra["C2_cols8_one_rank"] = {k_: e[k_] for k_ in ("metric", "value", "unit", "ms_per_step", "dtype", "config", "phases_ms", "roofline") if k_ in e}
                single = out["ms_per_step"]
                extra["C2_cols8_one_rank"]["projected_8_gpu_speedup_before_the_all_reduce"] = 8.0 * single / e["ms_per_step"]
                extra["C2_cols8_one_rank"]["wall_s"] = round(time.perf_counter() - t_extra, 1)
            except Exception as exc:   # noqa: BLE001 -- reported in the line
                extra["C2_cols8_one_rank"] = {"error": f"{type(exc).__name__}: {exc}"}
        if extra:
            out["extra_configs"] = extra
        print(json.dumps(out), flush=True)
    if ctx.dist is not None:
        ctx.dist.barrier()
        ctx.dist.destroy_process_group()


def run_config(args, ctx):
    """One configuration, end to end: tables, step loop, warmup, the timed repetitions, the per-phase pass, evaluate() and the
    CPU baselines.  Returns the JSON object of the line (rank 0; None elsewhere)."""
    world, rank, dist, backend = ctx.world, ctx.rank, ctx.dist, ctx.backend
    from ampligraph_amd.datasets import make_synthetic_kg
    from ampligraph_amd.engine import KgeEngine
    from ampligraph_amd.latent_features import loss_functions, optimizers
    from ampligraph_amd.trainer import StepLoop

    if os.environ.get("AMDKGE_RANK_EARLY"):   # development: "on,check_l1,check_rot,cost" of the distance models' early exit (amdkge_set_rank_early)
        from ampligraph_amd import _ffi as _f

        _f.check(_f.lib().amdkge_set_rank_early(*([int(v) for v in os.environ["AMDKGE_RANK_EARLY"].split(",")] + [-1])[:5]))
    if os.environ.get("AMDKGE_TILE_DIRECT", "1") == "0":   # development A/B: long rows on the LDS-accumulator tile kernel
        from ampligraph_amd import _ffi as _f

        _f.lib().amdkge_set_tile_direct(0)
    stream = SYNTH_STREAM.get(args.dataset)
    if stream is not None:     # no host-side triples at all: (s, p, o) number i comes from the counter RNG on the device
        N, R = (args.ents_per_gpu or stream["ents_per_gpu"]) * world, stream["n_rels"]
        data = {"n_ents": N, "n_rels": R, "train": None, "valid": None, "test": None}
    else:
        data = make_synthetic_kg(args.dataset, seed=0, popularity=args.popularity)
        N, R = data["n_ents"], data["n_rels"]
    cols = args.parallelism == "columns"
    cols_w = (args.cols_of or world) if cols else 1   # ranks of the column-sharded run this process is one rank of
    sharded = args.parallelism != "replicated" and ctx.multi and not cols
    rng = np.random.Generator(np.random.PCG64(0))
    Kf = 2 * args.k if args.model in ("ComplEx", "HolE", "RotatE") else args.k
    lim_e, lim_r = float(np.sqrt(6.0 / (N + Kf))), float(np.sqrt(6.0 / (R + Kf)))
    big = N * Kf > 400_000_000   # > 1.6 GB tables: initialise on the device (no CPU baseline / oracle at that size)
    ent0 = None if big else rng.uniform(-lim_e, lim_e, size=(N, Kf)).astype(np.float32)  # Glorot uniform, same on every rank
    rel0 = rng.uniform(-lim_r, lim_r, size=(R, Kf)).astype(np.float32)
    opt = optimizers.get("adam")
    opt.lazy = args.optimizer_mode == "lazy"
    rows_held = N   # entity rows this rank's table holds (row-sharded: its shard)

    def fill_rows(eng, lo, hi):
        """rows [lo, hi) of the whole-table initial values into eng.ent[0 : hi - lo] (host draw for small tables, a seeded
        device draw per rank for tables that do not fit host RAM), always through pack(): the stored layout may be padded"""
        if ent0 is not None:
            eng.pack(ent0[lo:hi], out=eng.ent[:hi - lo])
            return
        g = torch.Generator(device="cuda").manual_seed(1 + rank)
        step = max(1, (1 << 28) // Kf)
        for r0 in range(0, hi - lo, step):
            r1 = min(hi - lo, r0 + step)
            eng.pack((torch.rand(r1 - r0, Kf, device="cuda", generator=g) * 2 - 1) * lim_e, out=eng.ent[r0:r1])

    if cols:
        from ampligraph_amd.colsharded import ColumnStepLoop, check_columns, column_slice

        check_columns(args.model, args.k, cols_w)
        if cols_w != world and world != 1:
            raise SystemExit("--cols-of is a ONE-GPU measurement of one rank's share; with --gpus N the run is N-way column-sharded")
        eng = KgeEngine(args.model, args.k // cols_w, N, R, max_rel_size=R, k_full=args.k)
        eng.pack(column_slice(ent0, args.model, args.k, cols_w, rank), out=eng.ent)
        eng.pack(column_slice(rel0, args.model, args.k, cols_w, rank), out=eng.rel)
        loop = ColumnStepLoop(eng, args.eta, loss_functions.get(args.loss), opt, None, seed=0, dist=dist)
    elif sharded:
        from ampligraph_amd.sharded import ShardedStepLoop, ShardSpec

        negs = args.parallelism.split("-")[1]
        spec = ShardSpec(N, world, rank)
        # the synthetic graphs are uniform over the ids BY CONSTRUCTION: request lists at twice the even split (the product's
        # default is the worst case, right for first-seen ids in sequential batches; --popularity zipf keeps it)
        cap_factor = 2.0 if args.popularity == "uniform" else None
        cap = ShardedStepLoop.rows_needed(args.batch, args.eta, negs, world, N, cap_factor=cap_factor)
        cap_default = ShardedStepLoop.rows_needed(args.batch, args.eta, negs, world, N)   # what the product sizes the lists at
        eng = KgeEngine(args.model, args.k, spec.n_local + cap, R, max_rel_size=R)
        rows_held = spec.n_local
        fill_rows(eng, spec.lo, spec.hi)
        eng.pack(rel0, out=eng.rel)
        loop = ShardedStepLoop(eng, spec, args.eta, loss_functions.get(args.loss), opt, None, 0, dist, negatives=negs)
    else:
        eng = KgeEngine(args.model, args.k, N, R, max_rel_size=R)
        fill_rows(eng, 0, N)
        eng.pack(rel0, out=eng.rel)
        # the product's own step loop (what ScoringBasedEmbeddingModel.fit drives)
        loop = StepLoop(eng, args.eta, loss_functions.get(args.loss), opt, None, seed=0, dist=dist)

    B = args.batch
    Bg = B * (cols_w if cols else world)
    loop.deterministic = bool(args.deterministic) or loop.deterministic
    if hasattr(loop, "configure_for_data") and data["train"] is not None:
        loop.configure_for_data(data["train"], Bg)
    if args.skew_mode != "auto" and hasattr(loop, "pos_atomic"):
        from ampligraph_amd.trainer import HOT_ROW_REPLICA_THRESHOLD, hot_rows

        loop.pos_atomic = args.skew_mode == "atomic"
        eng.set_hot_rows(hot_rows(data["train"], B, HOT_ROW_REPLICA_THRESHOLD)[0] if args.skew_mode == "hot" else None)
    # the training set lives in HBM; a global batch is a contiguous slice (reference order: sequential,
    # un-shuffled, graph_data_loader.py:472-523); each rank takes its share of it inside the step loop
    if stream is None:
        train = torch.as_tensor(data["train"]).cuda()
        steps_per_epoch = max(1, train.shape[0] // Bg)

        def batch_of(step):
            b0 = (step % steps_per_epoch) * Bg
            return train[b0:b0 + Bg]
    else:
        stream_buf = torch.empty(Bg, 3, dtype=torch.int32, device="cuda")

        def batch_of(step):   # triples [step * Bg, (step + 1) * Bg) of the 500 M-triple stream, generated in place (one launch)
            return eng.synth_triples(0, step * Bg, Bg, N, R, out=stream_buf)

    # N > 1, replicated tables: which gradient-merge schedule is fastest depends on the fabric -- measure the candidates
    # on this node first (ordinary training steps, before the warmup; AMDKGE_DP_MERGE pins one instead)
    tuned = 0
    if ctx.multi and not sharded and not cols and "AMDKGE_DP_MERGE" not in os.environ and not opt.lazy:
        tuned = loop.tune_merge(batch_of, 0)
    loop.kernel_hook = None
    loop.reset_loss()
    nxt = tuned
    for _ in range(args.warmup):
        loop.step(batch_of(nxt), nxt)
        nxt += 1
    # ---- timed: `reps` repetitions of EXACTLY `steps` steps, each bracketed by barrier + synchronize on both sides; nothing but
    #      the step calls inside (no event records, no host reads); max over ranks per repetition, median repetition reported
    rep_s = []
    for _ in range(max(1, args.reps)):
        torch.cuda.synchronize()
        if ctx.multi:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _s in range(args.steps):
            loop.step(batch_of(nxt), nxt)
            nxt += 1
        torch.cuda.synchronize()
        if ctx.multi:
            dist.barrier()
        torch.cuda.synchronize()
        rep_s.append(time.perf_counter() - t0)
    rank_ms = [float(np.median(rep_s)) / max(1, args.steps) * 1e3]   # this rank's median, before the max over ranks
    if ctx.multi:
        t = torch.tensor(rep_s, dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        rep_s = [float(x) for x in t.tolist()]
        rk = torch.zeros(world, dtype=torch.float64, device="cuda")
        rk[rank] = rank_ms[0]
        dist.all_reduce(rk)
        rank_ms = [float(x) for x in rk.tolist()]
    dt = float(np.median(rep_s))
    loss_mean = loop.mean_batch_loss()
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, eng, rows_held, loss_mean)

    # ---- untimed (--full): the per-phase split, HIP events on the stream the kernels are launched on (torch's current stream)
    #      at the phase boundaries of the same step (single GPU: the kernel pair IS the step -- one phase)
    phases = list(loop.PHASES) if (ctx.multi or sharded or cols) else ["kernels"]
    n_ph = max(1, min(args.phase_steps, args.steps)) if (args.steps and args.full) else 0
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(loop.PHASES) + 1)] for _ in range(n_ph)]
    cur = {"i": None}

    def hook(i):
        if cur["i"] is not None:
            ev[cur["i"]][i].record()

    loop.kernel_hook = hook
    for i in range(n_ph):
        cur["i"] = i
        loop.step(batch_of(nxt), nxt)
        nxt += 1
    cur["i"] = None
    loop.kernel_hook = None
    torch.cuda.synchronize()
    if ctx.multi:
        dist.barrier()
    phase_ms = {nm: float(np.mean([e[i].elapsed_time(e[i + 1]) for e in ev])) for i, nm in enumerate(phases)} if n_ph else {}
    kern_ms = phase_ms.get("kernels", float("nan"))
    if cols and phase_ms:   # this rank's kernels: everything but the exchange
        kern_ms = phase_ms["partial scores"] + phase_ms["loss + stage + tiles"]
    out = None
    if rank == 0:
        triples = float(Bg if cols else world * B) * (1 + args.eta) * args.steps
        backend_world = dist.get_world_size() if ctx.multi else 1
        bytes_per_pos = 2.0 * (3 + args.eta) * 4.0 * eng.K   # each distinct row read once + its gradient written once
        Bw = Bg if cols else B   # positives this rank's kernels process per step
        achieved = bytes_per_pos * Bw / (kern_ms * 1e-3) / 1e9
        # PMC traffic cannot be collected inside this process (rocprofv3 wraps the command): the figure below is REPLAYED from
        # the committed counter passes of the headline workload (scripts/profile_bench.sh) and labelled as such; null otherwise
        traffic, traffic_source = None, None
        if args.full and not ctx.multi and not cols and args.preset == "C2" and args.popularity == "uniform" and not opt.lazy and not loop.deterministic:
            for cand in ("r06_pmc_traffic.json", "r05_pmc_traffic.json", "r04_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json", "pmc_traffic.json"):
                pmc = os.path.join(ROOT, "profiles", cand)
                if os.path.exists(pmc):
                    try:
                        traffic = json.load(open(pmc)).get("train_step_hbm_bytes_per_launch")
                        traffic_source = f"replayed from profiles/{cand} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload; not measured in this run)"
                    except Exception:
                        traffic = None
                    break
        tiled = loop.use_tiled and eng.tiled_supported(B, args.eta)
        kernel_names = (["train_fwdbwd_kernel<..., STAGE=true>", "tile_backward_kernel"] if tiled else ["train_fwdbwd_kernel"])
        if cols:
            kernel_names = ["cols_scores_kernel", "cols_loss_kernel", "cols_stage_kernel", "tile_backward_kernel"]
        opt_bytes = 7.0 * 4.0 * eng.K * (N + R) if ((not ctx.multi or cols) and not opt.lazy) else None
        opt_txt = ("dense (non-lazy) Keras-legacy Adam every step" if not opt.lazy else
                   "touched-rows (lazy) Adam: a documented deviation from the reference's dense optimizer")
        if cols:
            par = (f"cols{cols_w} (COLUMN-sharded tables: this rank holds {args.k // cols_w} of the {args.k} units of every row and processes the "
                   f"whole global batch of {Bg} positives; one all-reduce of {Bg * (1 + args.eta) * 4 / 1e6:.1f} MB of partial scores per step"
                   + (f"; ONE rank of {cols_w} measured on one GPU, the all-reduce through {'a one-rank ' + str(dist.get_backend()) + ' group' if ctx.multi else 'no process group (skipped)'}" if cols_w != world else "") + ")")
        elif sharded:
            par = (f"rows{world} (row-sharded entity table, {args.parallelism.split('-')[1]} negatives, device-side routing, "
                   f"equal-split all_to_all row / gradient exchange, {loop.cap_peer} request slots per peer"
                   f"{' = cap_factor 2.0 for the uniform synthetic ids' if cap_factor else ''}; the product's default "
                   f"(worst case) is {cap_default // world}))")
        elif ctx.multi:
            par = (f"dp{world} (replicated tables, gradient merge: {getattr(loop, 'merge', 'allreduce')}"
                   f"{'/' + loop.collectives if getattr(loop, 'merge', '') == 'sharded' else ''})")
        else:
            par = "single GPU"
        headline = args.preset == "C2" and not (cols and cols_w != world)
        out = {
            "metric": ("training triples/sec (incl. negatives), ComplEx k=200 eta=20 FB15K-237-shaped" if headline
                       else (f"ONE RANK's share of a {cols_w}-way column-sharded step, measured on one GPU: triples/sec (incl. negatives) of the GLOBAL "
                             f"batch through this rank's kernels, {args.model} k={args.k} eta={args.eta} {args.dataset} -- NOT a {cols_w}-GPU measurement"
                             if cols and cols_w != world else
                             f"training triples/sec (incl. negatives), {args.model} k={args.k} eta={args.eta} {args.dataset}")),
            "value": triples / dt, "unit": "triples/s", "n_gpus": backend_world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            # the timed K-step region is repeated; value / ms_per_step are the median repetition (max over ranks each)
            "repetitions": len(rep_s), "ms_per_step_min": min(rep_s) / args.steps * 1e3, "ms_per_step_max": max(rep_s) / args.steps * 1e3,
            "ranks": {"backend": (dist.get_backend() if ctx.multi else None), "world": backend_world, "gpus_visible": torch.cuda.device_count(),
                      "ms_per_step_rank_min": min(rank_ms), "ms_per_step_rank_max": max(rank_ms), "rccl_version": ctx.rccl,
                      "forced_single_rank_group": ctx.forced,
                      "merge_schedule": ((f"{loop.merge}/{loop.collectives}" if getattr(loop, "merge", "") == "sharded" else getattr(loop, "merge", None))
                                         if (ctx.multi and not sharded) else None),
                      "request_slots_per_peer": ({"used": loop.cap_peer, "product_default": cap_default // world} if sharded else None)},
            "config": {"workload": f"{args.dataset} ({args.popularity}, seed 0) {args.model} k={args.k} eta={args.eta} "
                                   f"{args.loss} adam lr=1e-3, {B} positives/GPU/step, tables resident in HBM, {opt_txt}",
                       "preset": args.preset, "optimizer_mode": args.optimizer_mode, "deterministic": bool(loop.deterministic),
                       "global_batch": Bg, "n_ents": N, "n_rels": R, "row_floats": eng.K, "stored_row_floats": eng.Ks,
                       "parallelism": par, "merge_ms_per_step_measured": getattr(loop, "merge_report", None)},
            "mean_batch_loss": loss_mean,
            "phases_ms": phase_ms,
            "roofline": {"bound": "hbm", "kernel": " + ".join(kernel_names), "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                         "kernel_ms": kern_ms, "algorithmic_bytes_per_launch": bytes_per_pos * Bw,
                         # SURVEY.md 8(d) reports the optimizer separately: 7*4K bytes per updated row (x, m, v read + written, g
                         # read).  Known on the host only for the dense mode on one GPU, where the pair sweeps every row
                         "optimizer_bytes_per_launch": opt_bytes,
                         "frac_incl_optimizer": ((bytes_per_pos * Bw + opt_bytes) / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS
                                                 if opt_bytes is not None and tiled else None),
                         "kernel_ms_source": f"HIP events on the launch stream around the pair, mean of {n_ph} steps recorded right after "
                                             "the timed repetitions (same workload, same process; the timed region itself holds no event records)",
                         "note": "launch = one train step's kernel pair (HIP events on the launch stream around both); "
                                 "single GPU: the pair also applies the optimizer (7*4K*(N+R) B/step dense), which is NOT counted "
                                 "in the algorithmic bytes; traffic = L2<->fabric bytes (PMC, Infinity-Cache hits included)"},
        }
        if not args.full:   # both come from the per-phase pass of --full
            del out["phases_ms"], out["roofline"]
        if args.full and not ctx.multi and not args.no_eval and data["test"] is not None:
            out["eval"] = eval_bench(eng, data, rank)
            if args.preset == "C2" or args.trained_eval:
                # the same evaluation on TRAINED-LIKE tables (VERDICT r3 #10 iv): untrained tables are the kindest case for the
                # screening pass's recheck list and the unkindest for the distance models' early exit
                if args.model in ("TransE", "RotatE"):
                    planted = plant_fitted_triples(eng, data, args.model, args.k)
                    e2 = eval_bench(eng, data, rank, triples=planted, filter_sets=[planted])
                    e2["how"] = ("planted: the object rows of these triples set to the model's prediction (s + p resp. s o r) + noise of half the "
                                 "table's std -- the tables of a fitted model, without training (the synthetic graph has nothing to learn)")
                else:
                    keep_lr = opt.learning_rate
                    opt.learning_rate = 1e-2
                    for _ in range(300):
                        loop.step(batch_of(nxt), nxt)
                        nxt += 1
                    opt.learning_rate = keep_lr
                    torch.cuda.synchronize()
                    e2 = eval_bench(eng, data, rank, triples=data["train"][:data["test"].shape[0]])
                    e2["how"] = "300 more steps of the same workload at lr 1e-2, evaluated on the first n_test TRAINING triples (filter = train + valid + test)"
                out["eval_trained_like"] = {k_: e2[k_] for k_ in ("ranks_per_s", "ranks_per_s_incl_filter_build", "ms", "n_test", "screening", "exact_fp32_kernel_alone", "roofline", "mrr_untrained_tables", "how") if k_ in e2}
                out["eval_trained_like"]["mrr"] = out["eval_trained_like"].pop("mrr_untrained_tables")
        if (args.full and not ctx.multi and not cols and not args.no_eval and data["train"] is not None and not big and not opt.lazy and not loop.deterministic
                and (args.preset == "C2" or args.dropin)):
            try:
                d_in = dropin_bench(args, data, dt / args.steps * 1e3, out.get("eval", {}).get("ms"))
                out["dropin"] = d_in
                # the two figures the verdict asks for, beside `value` / `eval` at the top level of the line
                out["fit_epoch_ms"], out["evaluate_call_ms"] = d_in["fit_epoch_ms"], d_in["evaluate_call_ms"]
            except Exception as exc:   # noqa: BLE001 -- reported, never costs the headline line
                out["dropin"] = {"error": f"{type(exc).__name__}: {exc}"}
        if args.full and not ctx.multi and not args.no_cpu_baseline and not big and data["train"] is not None and not opt.lazy:
            out["cpu_baseline"] = cpu_baseline(args, data, ent0, rel0)
            if not args.no_eval and data["test"] is not None:
                out["cpu_baseline"]["eval"] = cpu_eval_baseline(args, data, ent0, rel0)
    return out


if __name__ == "__main__":
    main()

"""Time of ranking against per-triple candidate lists (KgeEngine.rank_lists, amdkge_rank_lists) beside the only way to get those
ranks in bulk without it: ComplEx k = 200, n = 4 096 test triples x C = 500 candidates per side, both sides, filtered, "worst" --
at N = 14 541 entities (FB15K-237's table: cache-resident) and N = 1 000 000 (a 1.6 GB table: the gathers come from HBM).

Baseline (only calls that exist without rank_lists, same process): materialise the n x C corrupted triples of a side on the
device, KgeEngine.score them, quantise as the rank kernels do (int32(score * 1000), truncation) and count against the quantised
positive score with torch comparisons; a known positive that outranks is taken out with a precomputed boolean mask (the mask is
built outside the timed region: that favours the baseline).  It reads three rows per pair and writes n x C scores where rank_lists
reads one row per pair.

The tables are DYADIC (entries j / 8, j in -4 .. 4): every product and partial sum is exact in fp32 whatever its order, so
KgeEngine.score's lane-strided sum and the rank kernels' unit-order chain give the same bits and the two paths' ranks must be
EQUAL -- the script asserts it.  Neither path's work depends on the values.

Method: warm-up of both paths, then `--reps` timed regions per path, the two paths alternating, each region `--inner` back-to-back
calls between two device events (a call is about a millisecond); per-call time = region / inner; the median over the regions, and
min .. max as the spread.  The filter ranges (device index, amdkge_filter_ranges) are looked up before the timed
regions.  Effective gather rate = 2 sides x n x C x 1 600 B / time, beside the MI355X's 8 TB/s HBM peak.

    python scripts/bench_candidates.py [--reps 9] [--inner 20] [--sizes 14541,1000000] [--out profiles/candidates_eval.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ampligraph_amd import _ffi  # noqa: E402
from ampligraph_amd.engine import KgeEngine  # noqa: E402

HBM_PEAK_TBS = 8.0


def dyadic_fill_(t, gen):
    """t <- j / 8, j uniform in -4 .. 4, in row chunks (the 1 000 000-row table is 1.6 GB)"""
    step = 1 << 17
    for r0 in range(0, t.shape[0], step):
        blk = t[r0:r0 + step]
        blk.copy_(torch.randint(-4, 5, blk.shape, generator=gen, device=t.device, dtype=torch.int32).to(torch.float32) / 8.0)


def timed(fn, inner):
    """seconds per call over a region of `inner` back-to-back calls between two device events, and the last call's result"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / inner, out


def stats(xs):
    xs = sorted(xs)
    return {"median_s": xs[len(xs) // 2], "min_s": xs[0], "max_s": xs[-1]}


def run_size(N, R, k, n, Cn, known_per_list, reps, inner, warmup, seed):
    dev = torch.device("cuda")
    eng = KgeEngine("ComplEx", k, N, R, max_rel_size=R)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    dyadic_fill_(eng.ent, gen)
    dyadic_fill_(eng.rel, gen)
    rng = np.random.default_rng(seed)
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1).astype(np.int32)
    blocks = {"s": rng.integers(0, N, (n, Cn)).astype(np.int32), "o": rng.integers(0, N, (n, Cn)).astype(np.int32)}
    # filter set: the test triples, and the first `known_per_list` candidates of every list as known positives of its triple
    F = [X]
    for col, sd in ((0, "s"), (2, "o")):
        A = np.repeat(X, known_per_list, 0)
        A[:, col] = blocks[sd][:, :known_per_list].reshape(-1)
        F.append(A)
    F = np.concatenate(F).astype(np.int32)
    Xd, Fd = torch.as_tensor(X).to(dev), torch.as_tensor(F).to(dev)
    off = np.arange(n + 1, dtype=np.int64) * Cn
    lo, hi = torch.as_tensor(off[:-1].copy()).to(dev), torch.as_tensor(off[1:].copy()).to(dev)
    sides = []
    for col, sd, side in ((0, "s", _ffi.SIDE_S), (2, "o", _ffi.SIDE_O)):
        keys, start, ids = eng.filter_build(Fd, sd, N, R)
        flt = eng.filter_ranges(keys, start, Xd, side, N, R) + (ids,)
        # the baseline's mask: candidate c of triple i is known iff the corrupted triple is in F (host, exact, not timed)
        other = 2 - col
        fkey = (F[:, 1].astype(np.int64) * N + F[:, other]) * N + F[:, col]
        ckey = ((X[:, 1].astype(np.int64) * N + X[:, other]) * N)[:, None] + blocks[sd]
        known = torch.as_tensor(np.isin(ckey, fkey)).to(dev)
        block = torch.as_tensor(blocks[sd]).to(dev)
        sides.append((col, side, (lo, hi, block.view(-1), Cn), flt, block, known))

    def new_path():
        out = torch.empty(n, 2, dtype=torch.int32, device=dev)
        for j, (_, side, cand, flt, _, _) in enumerate(sides):
            eng.rank_lists(Xd, side, cand, "worst", flt, out=out[:, j], out_stride=2)
        return out

    def baseline():
        out = torch.empty(n, 2, dtype=torch.int32, device=dev)
        qpos = (eng.score(Xd) * 1000.0).to(torch.int32)
        for j, (col, _, _, _, block, known) in enumerate(sides):
            T = Xd[:, None, :].expand(n, Cn, 3).contiguous()       # the n x C materialised triples of this side
            T[:, :, col] = block
            q = (eng.score(T.view(-1, 3)) * 1000.0).to(torch.int32).view(n, Cn)
            out[:, j] = ((q >= qpos[:, None]) & ~known).sum(1).to(torch.int32) + 1
        return out

    for _ in range(warmup):
        a, b = new_path(), baseline()
    torch.cuda.synchronize()
    assert torch.equal(a, b), ("ranks differ", int((a != b).sum()))
    t_new, t_base = [], []
    for _ in range(reps):
        t, a = timed(new_path, inner)
        t_new.append(t)
        t, b = timed(baseline, inner)
        t_base.append(t)
        assert torch.equal(a, b)
    sn, sb = stats(t_new), stats(t_base)
    pair_bytes = 2 * n * Cn * eng.Ks * 4
    res = {"n_ents": N, "table_bytes": N * eng.Ks * 4, "rank_lists": sn, "baseline_score_and_compare": sb,
           "speedup_of_medians": sb["median_s"] / sn["median_s"],
           "ranks_per_s": 2 * n / sn["median_s"], "baseline_ranks_per_s": 2 * n / sb["median_s"],
           "gather_bytes": pair_bytes, "gather_tb_per_s": pair_bytes / sn["median_s"] * 1e-12, "hbm_peak_tb_per_s": HBM_PEAK_TBS,
           "filter_hits_subtracted": int(sum(int(s[5].sum()) for s in sides)), "ranks_equal": True,
           "mean_rank": float(a.float().mean())}
    spread = (sn["max_s"] - sn["min_s"]) + (sb["max_s"] - sb["min_s"])
    res["faster_by_more_than_the_spread"] = bool(sb["median_s"] - sn["median_s"] > spread)
    del eng
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="14541,1000000")
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--n-rels", type=int, default=237)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--candidates", type=int, default=500)
    ap.add_argument("--known", type=int, default=5, help="candidates per list that are known positives of their triple")
    ap.add_argument("--reps", type=int, default=9, help="timed regions per path")
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls per timed region (a call is ~1 ms: one alone times the clock ramp)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_candidates needs a GPU: a time taken anywhere else says nothing")
    res = {"model": "ComplEx", "k": a.k, "n_rels": a.n_rels, "queries": a.queries, "candidates_per_side": a.candidates,
           "sides": 2, "strategy": "worst", "filtered": True, "reps": a.reps, "calls_per_region": a.inner, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "sizes": [run_size(int(N), a.n_rels, a.k, a.queries, a.candidates, a.known, a.reps, a.inner, a.warmup, seed=0) for N in a.sizes.split(",")]}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    slow = [s["n_ents"] for s in res["sizes"] if not s["faster_by_more_than_the_spread"]]
    if slow:
        raise SystemExit(f"rank_lists is not faster than the baseline by more than the spread at N = {slow}")


if __name__ == "__main__":
    main()

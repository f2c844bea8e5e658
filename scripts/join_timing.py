"""Device time of the self-join entry points of find_duplicates (amdkge_join_nearest / amdkge_join_radius, kge_join.hip) at the two
shapes of DESIGN.md section 3: n = 14 505, d = 400 (FB15K-237's entities, ComplEx k = 200) and n = 272 115, d = 1 200 (its training
triples, [s | p | o]).  Gaussian rows; warm-up, then the median of repeated runs between device events.  Prints one JSON line per
shape and entry point: ms, and the fraction of the pair-element ceiling (n (n - 1) / 2 * d pair-elements, each a subtract and an
FMA, at the 157.3 TF fp32 vector peak = 3.93e13 pair-elements/s).

    python scripts/join_timing.py [--reps 5] [--shapes 14505x400,272115x1200]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ampligraph_amd.engine import KgeEngine  # noqa: E402

CEILING = 157.3e12 / 4   # pair-elements/s: one packed subtract + one packed FMA per two pair-elements


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="14505x400,272115x1200")
    a = ap.parse_args()
    eng = KgeEngine("DistMult", 4, 4, 2)
    g = torch.Generator(device="cuda").manual_seed(0)
    for shape in a.shapes.split(","):
        n, d = (int(v) for v in shape.split("x"))
        X = torch.randn(n, d, device="cuda", generator=g)
        dist = eng.join_nearest(X)[0]
        thr = float(torch.quantile(dist[:100000].double(), 0.01))   # a radius that keeps ~1 % of the rows
        pe = n * (n - 1) / 2 * d
        for name, fn in (("join_nearest", lambda: eng.join_nearest(X)), ("join_radius", lambda: eng.join_radius(X, thr))):
            ms = timed(fn, a.reps, a.warmup)
            print(json.dumps({"entry": name, "n": n, "d": d, "ms": round(ms, 3), "pair_elements_per_s": pe / (ms * 1e-3),
                              "fraction_of_ceiling": round(pe / (ms * 1e-3) / CEILING, 3)}), flush=True)


if __name__ == "__main__":
    main()

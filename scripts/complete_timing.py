"""Wall time of discovery.query_topn_batch at the headline shape (ComplEx k = 200, N = 14 505 entities, 237 relations): 10 000 (s, p)
queries, filtered with the synthetic training set, top_n = 10 -- beside the only route to such lists without it, a loop of
query_topn (one query per call, unfiltered), timed over the first 500 of the same queries.  The graph is uniform-random and the
tables are the ones a one-epoch fit leaves.  Warm-up, then the median of repeated runs (host clock around synchronised calls).
The selection kernel's share of the batched call is the sum of device-event intervals around amdkge_topk_rows_excluding over
one call, taken in runs of their own.  Prints one JSON line.

    python scripts/complete_timing.py [--reps 5] [--queries 10000] [--loop-queries 500] [--top-n 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ampligraph_amd import discovery  # noqa: E402
from ampligraph_amd.latent_features import ScoringBasedEmbeddingModel  # noqa: E402


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--top-n", type=int, default=10)
    ap.add_argument("--model", default="ComplEx")
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--n-ents", type=int, default=14505)
    ap.add_argument("--n-rels", type=int, default=237)
    ap.add_argument("--n-triples", type=int, default=272115)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--loop-queries", type=int, default=500)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    N, R, n = a.n_ents, a.n_rels, a.n_triples
    X = np.stack([rng.integers(0, N, n), rng.integers(0, R, n), rng.integers(0, N, n)], 1)
    X[:N, 0] = np.arange(N)          # every entity and relation occurs
    X[:R, 1] = np.arange(R)
    m = ScoringBasedEmbeddingModel(eta=2, k=a.k, scoring_type=a.model, seed=0)
    m.compile(optimizer="adam", loss="multiclass_nll")
    m.fit(X, batch_size=30000, epochs=1, verbose=False)
    Q = X[rng.choice(n, a.queries, replace=False)][:, :2]      # (s, p) of training statements: every query has known objects
    eng = m._engine

    def batched():
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = discovery.query_topn_batch(m, Q, top_n=a.top_n, corrupt_side="o", use_filter={"train": X})
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    batched()                                                          # warm-up (filter index, workspaces, code objects)
    t_batch = median([batched()[0] for _ in range(a.reps)])

    # the selection kernel's share: device events around every amdkge_topk_rows_excluding launch of one call
    inner = eng.topk_rows_excluding
    spans = []

    def timed(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = inner(*args, **kw)
        e1.record()
        spans.append((e0, e1))
        return out

    sel = []
    eng.topk_rows_excluding = timed
    try:
        for _ in range(a.reps):
            spans.clear()
            batched()
            sel.append(sum(e0.elapsed_time(e1) for e0, e1 in spans) * 1e-3)
        launches = len(spans)
    finally:
        del eng.topk_rows_excluding
    t_sel = median(sel)

    def loop():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for s, p in Q[:a.loop_queries]:
            discovery.query_topn(m, top_n=a.top_n, head=s, relation=p)
        torch.cuda.synchronize()
        return time.perf_counter() - t

    loop()
    t_loop = median([loop() for _ in range(a.reps)])
    print(json.dumps({"model": a.model, "k": a.k, "n_ents": N, "n_rels": R, "n_triples": n, "top_n": a.top_n, "reps": a.reps,
                      "queries": a.queries, "query_topn_batch_s": t_batch, "selection_kernel_s": t_sel, "selection_launches": launches,
                      "selection_share": t_sel / t_batch, "loop_queries": a.loop_queries, "query_topn_loop_s": t_loop,
                      "query_topn_loop_per_query_s": t_loop / a.loop_queries, "query_topn_batch_per_query_s": t_batch / a.queries,
                      "per_query_ratio": (t_loop / a.loop_queries) / (t_batch / a.queries)}), flush=True)


if __name__ == "__main__":
    main()
